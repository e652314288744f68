"""lgh_diagnostics / lgh_diagnostics_zones (Context.diagnostics, .diagnostics_zones): the conserved integrals, point
extremes and bad-point counts of a state, per zone and folded over zones and ranks, against the numpy restatement of
tests/diag_ref.py, the oracle's energies, and the edge states of tests/edge_states.py.

State of the numpy cases: curved mesh (x0 + 0.2 h rng), random v, e in [-0.5, 1] (negative point values occur), random
rho0_q in [0.5, 2] and a random gamma per zone; m_q is read back from the context (Context.rho0DetJ0w).  Shapes: those of
tests/test_gpu_sample.py - one zone, a few, more than one workgroup's worth in 1D, unequal zone counts per axis, 75 zones,
Q4Q3 in 2D - and 2 x 2 x 1 zones of Q5Q4 in 3D, whose 1000 points per zone are more than a workgroup (the point loop, and
one dof set at a time through the staging buffers).

Bounds (none taken from what the kernel gives):
  sums per zone      (NQ + dim D1D^dim + 8) 2^-52 sum_q |term|: NQ terms, each an interpolated value of dim D1D^dim
                     products, added in another order than numpy's;
  sums over zones    the same with NE in place of NQ, on the sum of the zones' |term| sums (the zone values themselves are
                     the kernel's own: only the fold is compared);
  point extremes     relative max(1e-13, 2 eps kappa), kappa the condition of detJ as data formed from J = sum G x
                     (diag_ref.py);
  counts             exact - the reference alone is first checked to hold no detJ_q within 1e-9 max|detJ| of 0 and no e_q
                     within 1e-12 of 0, so no count hangs on a rounding;
  oracle energies    ie and ke against the oracle: both sides are sums of NE NQ terms in their own order, twice the sum
                     bound with NE NQ terms; mass against numpy's sum and volume against the domain's exact volume: the sum
                     bound itself."""
import os
import threading

import numpy as np
import pytest

from diag_ref import COUNTS, MAXS, MINS, NAMES, SUMS, diag_reference

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
ZONES = {"1D-1": (1,), "1D-3": (3,), "1D-257": (257,), "2D-3x2": (3, 2), "3D-3x2x2": (3, 2, 2), "3D-5x5x3": (5, 5, 3),
         "3D-2x2x1": (2, 2, 1)}
ORDERS = [(1, 0), (2, 1), (3, 2)]
CASES = [(z, o) for z in list(ZONES)[:6] for o in ORDERS] + [("2D-3x2", (4, 3)), ("3D-2x2x1", (5, 4))]
IDS = [f"{z}-Q{o[0]}Q{o[1]}" for z, o in CASES]


class Case:
    """One discretisation with a context on the GPU, set up, and a random state on a curved mesh; the numpy reference is
    computed once, shared and never written."""

    def __init__(self, zones, ok, ot, renumber=None, take=None):
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
        self.dim, self.NE, self.N, self.D, self.L, self.Q = dim, int(np.prod(zones)), N, ok + 1, ot + 1, B.shape[0]
        self.h1map, self.W, self.B, self.G, self.Bl = h1map, np.asarray(W), B, G, Bl
        NE, NL, H1V = self.NE, self.L ** dim, dim * N
        self.NQ, self.ND = self.Q ** dim, self.D ** dim
        rng = np.random.default_rng(1000 * dim + 10 * ok + NE)
        hmin = 1.0 / (max(zones) * ok)
        self.x0 = x0
        self.S = np.concatenate([x0 + 0.2 * hmin * rng.uniform(-1, 1, H1V),      # curved zones
                                 rng.uniform(-1, 1, H1V), rng.uniform(-0.5, 1.0, NE * NL)])
        self.rho0_l2 = rng.uniform(0.5, 2.0, NE * NL)
        self.rho0_q = rng.uniform(0.5, 2.0, NE * self.NQ)
        self.gamma = rng.uniform(1.2, 1.8, NE)
        if take is not None:   # the same data in another numbering
            self.x0, self.S, self.rho0_l2, self.rho0_q, self.gamma = take
        self.ctx = Context(dim, NE, self.D, self.Q, self.L, N, h1map, B, G, Bl, W, self.gamma, ess, order_v=ok)
        self._ref = None

    def setup(self):
        c = self.ctx
        c.setup_rho0detj0(c.to_dev(self.x0), c.to_dev(self.rho0_l2), c.to_dev(self.rho0_q))
        self.m = c.rho0DetJ0w
        self.Sd = c.to_dev(self.S)
        return self

    def reference(self, S=None):
        if S is not None:
            return diag_reference(self.dim, self.NE, self.N, self.D, self.L, self.h1map, S, self.m, self.gamma, self.W, self.B, self.G, self.Bl)
        if self._ref is None:
            self._ref = self.reference(self.S)
            for a in self._ref.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        return self._ref

    def zones(self, Sd=None):
        """the 17 zone arrays [17, NE]; NaN-filled before the call: an entry the kernel does not write shows"""
        out = self.ctx.to_dev(np.full(17 * self.NE, np.nan))
        self.ctx.diagnostics_zones(self.Sd if Sd is None else Sd, out)
        self.ctx.sync()
        return out.cpu().numpy().reshape(17, self.NE)

    def glob(self, Sd=None):
        """the 20 global figures; Context.diagnostics fills its array with NaN before the call"""
        return self.ctx.diagnostics(self.Sd if Sd is None else Sd, raw=True)

    def sum_bound(self, nterms):
        return (nterms + self.dim * self.ND + 8) * EPS

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(zones_id, order, renumber=None):
        key = (zones_id, order, renumber)
        if key not in made:
            made[key] = Case(ZONES[zones_id], order[0], order[1], renumber).setup()
        return made[key]
    yield get
    for c in made.values():
        c.close()


def check_reference_is_decided(ref):
    """no count of the reference hangs on a rounding"""
    det, e = ref["detJ"], ref["e"]
    assert np.abs(det).min() > 1e-9 * np.abs(det).max()
    assert np.abs(e).min() > 1e-12


def check_zones(c, got, ref, what=""):
    assert not np.isnan(got).any(), (what, "an entry was not written")
    zone = ref["zone"]
    for k in SUMS:
        err, bound = np.abs(got[k] - zone[k]), c.sum_bound(c.NQ) * ref["abs_zone"][k]
        print(f"{what} {NAMES[k]}: max err {err.max():.3e}, bound there {bound[np.argmax(err)]:.3e}")
        assert np.all(err <= bound), (what, NAMES[k], err.max())
    tol = max(1e-13, 2.0 * EPS * ref["kappa"])
    for k in MINS + MAXS:
        err = np.abs(got[k] - zone[k])
        worst = np.argmax(err - tol * np.abs(zone[k]))
        print(f"{what} {NAMES[k]}: err {err[worst]:.3e} at a value of {zone[k][worst]:.3e}, tol {tol:.3e} of it")
        assert np.all(err <= tol * np.abs(zone[k])), (what, NAMES[k], err[worst], zone[k][worst], tol)
    for k in COUNTS:
        assert np.array_equal(got[k], zone[k]), (what, NAMES[k])


def check_global_against_zones(c, g, z, ref, what=""):
    assert not np.isnan(g).any(), what
    for k in SUMS:
        bound = c.sum_bound(c.NE) * ref["abs_glob"][k]
        print(f"{what} global {NAMES[k]}: err {abs(g[k] - z[k].sum()):.3e}, bound {bound:.3e}")
        assert abs(g[k] - z[k].sum()) <= bound, (what, NAMES[k])
    for k in MINS:
        assert g[k] == z[k].min(), (what, NAMES[k])
    for k in MAXS:
        assert g[k] == z[k].max(), (what, NAMES[k])
    for k in COUNTS:
        assert g[k] == z[k].sum(), (what, NAMES[k])
    assert g[17] == int(np.argmin(z[7])) and g[18] == 0 and g[19] == 0, (what, g[17:])


@pytest.mark.parametrize("zones_id,order", CASES, ids=IDS)
def test_zones_match_numpy(cases, zones_id, order):
    c = cases(zones_id, order)
    ref = c.reference()
    check_reference_is_decided(ref)
    if c.NE >= 12:   # negative point energies occur: the clamp of the pressure and the count are in play
        assert ref["glob"][15] > 0 and ref["glob"][15] < c.NE * c.NQ
    check_zones(c, c.zones(), ref, f"{zones_id} Q{order[0]}Q{order[1]}")


@pytest.mark.parametrize("zones_id,order", CASES, ids=IDS)
def test_global_is_the_fold_of_the_zones(cases, zones_id, order):
    c = cases(zones_id, order)
    ref = c.reference()
    g, z = c.glob(), c.zones()
    check_global_against_zones(c, g, z, ref, f"{zones_id} Q{order[0]}Q{order[1]}")
    # and against the reference as a whole
    for k in SUMS:
        assert abs(g[k] - ref["glob"][k]) <= (c.sum_bound(c.NQ) + c.sum_bound(c.NE)) * ref["abs_glob"][k], NAMES[k]
    for k in COUNTS:
        assert g[k] == ref["glob"][k], NAMES[k]


@pytest.mark.parametrize("zones_id,order", [("1D-257", (3, 2)), ("2D-3x2", (4, 3)), ("3D-5x5x3", (3, 2)), ("3D-2x2x1", (5, 4))])
def test_same_bits_every_time(cases, zones_id, order):
    c = cases(zones_id, order)
    alone = c.zones()
    g1 = c.glob()
    after = c.zones()                       # right after the global call
    g2 = c.glob()
    assert np.array_equal(alone.view(np.uint64), after.view(np.uint64))
    assert np.array_equal(alone.view(np.uint64), c.zones().view(np.uint64))
    assert np.array_equal(g1.view(np.uint64), g2.view(np.uint64))


@pytest.mark.parametrize("renumber", ["random", "mfem"])
def test_outputs_sit_at_the_callers_zone_ids(cases, renumber):
    """3 x 2 x 2 zones under another numbering of nodes and zones: the library may walk the zones in an order of its own, the
    zone arrays are indexed by the caller's ids and slot 17 is one."""
    c = cases("3D-3x2x2", (3, 2), renumber)
    if renumber == "random":
        assert not np.array_equal(c.elem_perm, np.arange(c.NE))
    assert not np.array_equal(c.node_perm, np.arange(c.N))
    ref = c.reference()
    check_reference_is_decided(ref)
    got = c.zones()
    check_zones(c, got, ref, renumber)
    g = c.glob()
    check_global_against_zones(c, g, got, ref, renumber)
    # the same data in the generator's numbering: zone j is the structured zone elem_perm[j], structured node i is node node_perm[i]
    inv = np.argsort(c.elem_perm)
    nodes = lambda a, ncomp: np.concatenate([a[k * c.N:(k + 1) * c.N][c.node_perm] for k in range(ncomp)])
    zones = lambda a, per: a.reshape(c.NE, per)[inv].reshape(-1)
    H1V, NL = 3 * c.N, c.L ** 3
    S_lex = np.concatenate([nodes(c.S[:2 * H1V], 6), zones(c.S[2 * H1V:], NL)])
    lex = Case(ZONES["3D-3x2x2"], 3, 2, take=(nodes(c.x0, 3), S_lex, zones(c.rho0_l2, NL), zones(c.rho0_q, c.NQ), c.gamma[inv])).setup()
    try:
        z_lex = lex.zones()
        g_lex = lex.glob()
        ref_lex = lex.reference()
    finally:
        lex.close()
    tol = max(1e-13, 2.0 * EPS * max(ref["kappa"], ref_lex["kappa"]))
    for k in SUMS:
        assert np.all(np.abs(got[k] - z_lex[k][c.elem_perm]) <= c.sum_bound(c.NQ) * ref["abs_zone"][k]), NAMES[k]
    for k in MINS + MAXS:
        assert np.all(np.abs(got[k] - z_lex[k][c.elem_perm]) <= tol * np.abs(got[k])), NAMES[k]
    for k in COUNTS:
        assert np.array_equal(got[k], z_lex[k][c.elem_perm]), NAMES[k]
    assert c.elem_perm[int(g[17])] == int(g_lex[17])   # the same zone of the mesh, each in its caller's ids


def _fixed_boundary_state(prob, seed=3):
    """helpers.deformed_state with the boundary nodes left where they are: the domain keeps its volume"""
    from helpers import deformed_state
    S, S0 = deformed_state(prob, seed=seed), prob.initial_state()[0]
    X, X0 = S[:prob.H1V].reshape(prob.dim, prob.N), S0[:prob.H1V].reshape(prob.dim, prob.N)
    for e in prob.ess:
        idx = np.asarray(e, dtype=np.int64)
        X[:, idx] = X0[:, idx]
    return S


@pytest.mark.parametrize("mesh,order", [("square01_quad", (2, 1)), ("cube01_hex", (3, 2))], ids=["2D-Q2Q1", "3D-Q3Q2"])
def test_against_the_oracle(mesh, order):
    from helpers import make_gpu, make_oracle
    from oracle.fem import Problem
    prob = Problem(mesh=mesh, rs=1, order_v=order[0], order_e=order[1], problem=1)
    g, o = make_gpu(prob), make_oracle(prob)
    try:
        S = _fixed_boundary_state(prob)
        d = g.diagnostics(g.ctx.to_dev(S))
        m = g.ctx.rho0DetJ0w
        ref = diag_reference(prob.dim, prob.NE, prob.N, prob.D1D, prob.L1D, np.asarray(prob.h1map).reshape(-1), S, m, prob.initial_state()[2],
                             prob.W, prob.B, prob.G, prob.Bl)
        nterms = prob.NE * prob.NQ
        bound = lambda k: (nterms + prob.dim * prob.ND + 8) * EPS * ref["abs_glob"][k]
        ie, ke = o.internal_energy(S), o.kinetic_energy(S)
        print(f"ie {d['ie']!r} oracle {ie!r} bound {2 * bound(2):.3e}; ke {d['ke']!r} oracle {ke!r} bound {2 * bound(3):.3e}")
        assert abs(d["ie"] - ie) <= 2 * bound(2) and abs(d["ke"] - ke) <= 2 * bound(3)   # (the oracle's sum has its own order)
        assert abs(d["mass"] - m.sum()) <= bound(0)
        volume = float(np.prod([b[-1] - b[0] for b in prob.gbreaks]))
        print(f"volume {d['volume']!r} domain {volume!r} bound {bound(1):.3e}")
        assert abs(d["volume"] - volume) <= bound(1)
        assert d["n_inverted"] == d["n_nonfinite"] == d["n_negative_e"] == 0 and d["detj_min"] > 0
    finally:
        g.close()
        o.close()


BREAKS3 = [[0, .3, .7, 1], [0, .5, 1], [0, .4, 1]]          # 12 zones


@pytest.fixture(scope="module")
def edge():
    from helpers import make_gpu
    from oracle.fem import Problem
    prob = Problem(breaks=BREAKS3, order_v=2, order_e=1, problem=1)
    g = make_gpu(prob)
    m = g.ctx.rho0DetJ0w

    def run(S):
        Sd = g.ctx.to_dev(S)
        out = g.ctx.to_dev(np.full(17 * prob.NE, np.nan))
        g.ctx.diagnostics_zones(Sd, out)
        glob = g.ctx.diagnostics(Sd, raw=True)
        ref = diag_reference(3, prob.NE, prob.N, prob.D1D, prob.L1D, np.asarray(prob.h1map).reshape(-1), S, m, prob.initial_state()[2],
                             prob.W, prob.B, prob.G, prob.Bl)
        return out.cpu().numpy().reshape(17, prob.NE), glob, ref
    yield prob, run
    g.close()


def test_edge_inverted_layer(edge):
    import edge_states as es
    prob, run = edge
    z, g, ref = run(es.edge_state(prob, "inverted_layer"))
    check_reference_is_decided(ref)
    assert ref["glob"][14] > 0 and g[14] == ref["glob"][14] and np.array_equal(z[14], ref["zone"][14])
    layer = np.nonzero(ref["zone"][14])[0]                 # the zones of the reflected layer
    assert g[7] < 0 and int(g[17]) in layer and g[7] == z[7].min()
    # density and pressure are taken without the inverted points: positive, and those of the reference
    tol = max(1e-13, 2.0 * EPS * ref["kappa"])
    for k in (8, 9, 12):
        r = ref["zone"][k]
        fin = np.isfinite(r)
        assert np.all(np.abs(z[k][fin] - r[fin]) <= tol * np.abs(r[fin])) and np.array_equal(z[k][~fin], r[~fin]), NAMES[k]
    assert g[8] > 0 and g[9] > 0 and g[12] >= 0
    full = layer[ref["zone"][14][layer] == prob.NQ]        # zones with every point inverted have no density at all
    assert np.all(np.isposinf(z[8][full])) and np.all(np.isneginf(z[9][full])) and np.all(np.isneginf(z[12][full]))


def test_edge_all_negative_e(edge):
    import edge_states as es
    prob, run = edge
    z, g, ref = run(es.edge_state(prob, "all_negative_e"))
    assert g[15] == prob.NE * prob.NQ and np.all(z[15] == prob.NQ)
    assert g[12] == 0.0 and np.all(z[12] == 0.0)
    assert g[11] < 0 and g[14] == 0 and g[16] == 0


def test_edge_still_cold(edge):
    import edge_states as es
    prob, run = edge
    z, g, ref = run(es.edge_state(prob, "still_cold"))
    for k in (3, 4, 5, 6, 13):                             # ke, momentum, v_max: exact zeros
        assert g[k] == 0.0 and np.all(z[k] == 0.0), NAMES[k]
    assert g[2] == 0.0 and g[10] == 0.0 and g[11] == 0.0 and g[15] == 0


def test_a_nan_stays_in_its_zone(cases):
    """one e dof of one zone is NaN: the L2 Bernstein basis is positive at every point, so every point of that zone is
    non-finite; the sums say so, the extremes of the other zones keep their bits"""
    c = cases("3D-3x2x2", (2, 1))
    clean = c.zones()
    bad = 5
    S = c.S.copy()
    S[2 * 3 * c.N + bad * c.L ** 3 + 1] = np.nan
    Sd = c.ctx.to_dev(S)
    z, g = c.zones(Sd), c.glob(Sd)
    assert z[16][bad] == c.NQ and z[16].sum() == c.NQ and g[16] == c.NQ
    assert np.isnan(z[2][bad]) and np.isnan(g[2])
    assert np.isposinf(z[10][bad]) and np.isneginf(z[11][bad])
    others = np.arange(c.NE) != bad
    for k in (10, 11):
        assert np.array_equal(z[k][others].view(np.uint64), clean[k][others].view(np.uint64)), NAMES[k]
    assert np.isfinite(g[11]) and g[11] == clean[11][others].max() and g[10] == clean[10][others].min()
    for k in (0, 1, 3, 4, 5, 6):                           # the sums that do not read e are those of the clean state
        assert np.array_equal(z[k].view(np.uint64), clean[k].view(np.uint64)), NAMES[k]


def test_nothing_else_moves():
    """a row taken between two steps must not change the next step: the quadrature data, its generation counter, the fused
    force products and dt_est are as lgh_qupdate left them"""
    from helpers import deformed_state, make_gpu
    from oracle.fem import Problem
    prob = Problem(mesh="cube01_hex", rs=1, order_v=3, order_e=2, problem=1)
    g = make_gpu(prob)
    try:
        ctx = g.ctx
        S = deformed_state(prob, seed=5)
        Sd = ctx.to_dev(S)
        ctx.set_dt_est(float("inf"))
        ctx.qupdate(Sd)
        ctx.sync()

        def products():
            f1, ftv = ctx.zeros(prob.H1V), ctx.zeros(prob.L2V)
            assert ctx.fused_force_mult(f1) and ctx.fused_force_mult_transpose(ftv)
            ctx.sync()
            return f1.cpu().numpy(), ftv.cpu().numpy()

        before = products()
        gen, dt = ctx.quadrature_generation(), ctx.get_dt_est()
        assert gen[1] == 1 and gen[2] == 1 and np.isfinite(dt)
        d = ctx.diagnostics(Sd)
        out = ctx.zeros(17 * prob.NE)
        ctx.diagnostics_zones(Sd, out)
        ctx.sync()
        assert d["mass"] > 0 and np.abs(out.cpu().numpy()).max() > 0
        assert ctx.quadrature_generation() == gen and ctx.get_dt_est() == dt
        assert np.array_equal(Sd.cpu().numpy(), S)
        after = products()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    finally:
        g.close()


def test_refused_before_the_setup():
    from laghos_amd._lib import LghError
    c = Case(ZONES["3D-3x2x2"], 2, 1)
    try:
        Sd = c.ctx.to_dev(c.S)
        out = c.ctx.zeros(17 * c.NE)
        with pytest.raises(LghError, match="error 1: .*lgh_setup_rho0detj0"):      # LGH_ERR_ARG
            c.ctx.diagnostics(Sd)
        with pytest.raises(LghError, match="error 1: .*lgh_setup_rho0detj0"):
            c.ctx.diagnostics_zones(Sd, out)
        c.ctx.sync()
        assert not out.cpu().numpy().any()                 # no kernel ran
        c.setup()
        assert c.ctx.diagnostics(c.Sd)["mass"] > 0         # and it is served afterwards
    finally:
        c.close()


MESH_3D = ["-dim", 3, "-nx", 4, "-ny", 2, "-nz", 2, "-Sx", 2, "-Sy", 1, "-Sz", 1]
MESH_2D = ["-dim", 2, "-nx", 4, "-ny", 2, "-Sx", 2, "-Sy", 1]


def test_two_emulated_ranks():
    """3D, 4 x 2 x 2 zones on two ranks: see _two_emulated_ranks"""
    _two_emulated_ranks(MESH_3D)


def test_two_emulated_ranks_2d():
    """the same on 2D blocks: 4 x 2 zones on two ranks (momentum has two components: p_z stays 0)"""
    _two_emulated_ranks(MESH_2D)


def _two_emulated_ranks(mesh_args):
    """3D, 4 x 2 x 2 zones, Q2Q1 on two ranks (threads, "LGHLOCAL" communicator).
    At the initial state (the same bits on every partition, so the point values are) against the one-rank run of the same
    problem: both ranks return the same array; sums to the sum bound, extremes and counts exactly; slot 18 is the rank whose
    own zone array holds the minimum at the zone of slot 17, the lowest such rank.
    After two steps (the fluid moves: every slot carries a value of its own through the reductions; the states of a one-rank
    run differ by then, in the last bits of the CG sums) against the two ranks' own zone arrays: sums to the sum bound with
    the number of zones as the number of terms, extremes and counts exactly, the owner as before."""
    import ctypes
    import torch
    from laghos_amd import _lib, host_lib
    from laghos_amd.context import DIAG_COUNT, DIAG_ZONE_COUNT
    dim = mesh_args[1]
    args = mesh_args + ["-rs", 0, "-p", 1, "-ok", 2, "-ot", 1, "-pa", "-tf", 1e9, "-ms", 10 ** 6, "-vs", 10 ** 9, "-q"]
    L = _lib.load()

    def look(sim):
        """(the global array, NaN-filled before the call; this rank's own zone arrays, through the sim's context)"""
        raw = np.full(DIAG_COUNT, np.nan)
        sim.L.laghos_sim_diagnostics(sim.h, raw.ctypes.data)
        ctx = ctypes.c_void_p(sim.L.laghos_sim_context(sim.h))
        S = torch.as_tensor(sim.state()).cuda()
        z = torch.full((DIAG_ZONE_COUNT * sim.sizes()["NE"],), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        _lib.check(L.lgh_diagnostics_zones(ctx, ctypes.c_void_p(S.data_ptr()), ctypes.c_void_p(z.data_ptr())))
        _lib.check(L.lgh_sync(ctx))
        return raw, z.cpu().numpy().reshape(DIAG_ZONE_COUNT, -1)

    def run(nranks, rank, cid, out, err):
        try:
            sim = host_lib.Sim(args, nranks=nranks, rank=rank, nccl_id=cid)
            sim.enable_timers(False)
            first = look(sim)
            for _ in range(2):
                assert sim.step() == 1
            out[rank] = (first[0], sim.sizes(), first[1], look(sim))
            sim.close()
        except Exception as ex:  # noqa: BLE001 - reported below
            err[rank] = repr(ex)

    one, err = {}, {}
    run(1, 0, None, one, err)
    assert not err, err
    cid = (b"LGHLOCAL" + os.urandom(16).hex().encode()).ljust(128, b"\0")
    two = {}
    th = [threading.Thread(target=run, args=(2, r, cid, two, err), daemon=True) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in th) and not err, err
    a, b, ref = two[0][0], two[1][0], one[0][0]
    assert not np.isnan(a).any() and not np.isnan(ref).any()          # every entry was written
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    sizes = one[0][1]
    assert two[0][1]["NE"] == two[1][1]["NE"] == sizes["NE"] // 2
    nterms, ND = sizes["global_NE"] * sizes["NQ"], sizes["D1D"] ** dim
    for k in SUMS:
        # every term of mass, volume, ie and ke is non-negative here, so sum |term| is the sum; the fluid is at rest: momentum is 0
        print(f"{NAMES[k]}: two ranks {a[k]!r}, one rank {ref[k]!r}")
        assert abs(a[k] - ref[k]) <= (nterms + 3 * ND + 8) * EPS * abs(ref[k]), NAMES[k]
    assert ref[0] > 0 and ref[1] > 0 and ref[2] > 0
    for k in MINS + MAXS + COUNTS:
        assert a[k] == ref[k], NAMES[k]

    def check_owner(g, zone_arrays):
        """the lowest rank whose zone array holds the minimum, and there the first such zone"""
        holders = [r for r in range(len(zone_arrays)) if zone_arrays[r][7].min() == g[7]]
        assert holders and g[18] == holders[0]
        assert g[17] == int(np.argmin(zone_arrays[holders[0]][7])) and g[19] == 0
    check_owner(a, [two[0][2], two[1][2]])
    check_owner(ref, [one[0][2]])
    # after two steps: the moving fluid, against the fold of the two ranks' own zone arrays
    g, g1 = two[0][3][0], two[1][3][0]
    assert not np.isnan(g).any() and np.array_equal(g.view(np.uint64), g1.view(np.uint64))
    z = np.concatenate([two[0][3][1], two[1][3][1]], axis=1)           # [17, global NE]
    assert g[3] > 0 and g[13] > 0 and all(g[k] != 0 for k in (4, 5, 6)[:dim])  # ke, v_max, momentum: values of their own
    for k in SUMS:
        print(f"after two steps, {NAMES[k]}: {g[k]!r}, sum of the zone arrays {z[k].sum()!r}")
        assert abs(g[k] - z[k].sum()) <= (sizes["global_NE"] + 3 * ND + 8) * EPS * np.abs(z[k]).sum(), NAMES[k]
    for k in MINS:
        assert g[k] == z[k].min(), NAMES[k]
    for k in MAXS:
        assert g[k] == z[k].max(), NAMES[k]
    for k in COUNTS:
        assert g[k] == z[k].sum(), NAMES[k]
    check_owner(g, [two[0][3][1], two[1][3][1]])
