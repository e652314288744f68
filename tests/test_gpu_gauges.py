"""lgh_gauges_* (Context.gauges_create / gauges_sample / gauges_pending / gauges_drain / gauges_mass / gauges_shape): the rows of a
set of gauges - material points (zone, xi) - against the numpy restatement of tests/gauges_ref.py, on the states, shapes and orders
of tests/test_gpu_sample.py (curved mesh, random v and e with negative values, a random gamma per zone), plus Q5Q4 on 3 x 2 x 2
zones: the largest LDS per gauge.

Tolerances.  x, v, e: TOL = 1e-13 (derived_ref.TOL, the project's figure for sums of at most D1D^dim products) of the largest dof
of the field.  detj and div_v: the per-point bounds of DESIGN.md §7f as tests/test_gpu_derived.py states them,
    |detj - ref| <= TOL |A_J|_F |J^-1|_F |det J|          |div_v - ref| <= dim TOL bound_L.
rho, p: EXACT relations on the GPU's own numbers, compared as uint64: rho is the one IEEE division m_g / detj, p the two products
(gamma - 1) rho max(e, 0).  cs: the bits lgh_sample_derived returns - at lattice points, and off them too, where the gauge's own table
rows are handed to that kernel as a lattice (derived_at) - and one spacing of numpy's square root (the device's square root is not
held to correct rounding: tests/test_gpu_derived.py).  A gauge at a lattice point, given that lattice's table rows, has the bits of
the dumps."""
import ctypes

import numpy as np
import pytest

import gauges_ref as gr
from derived_ref import TOL, lattice_tables3
from test_gpu_sample import ZONES, Case

pytestmark = pytest.mark.gpu

GRIDS = ["1D-1", "1D-257", "2D-3x2", "3D-3x2x2", "3D-5x5x3"]
ORDERS = [(1, 0), (2, 1), (3, 2)]
CASES = [(z, o) for z in GRIDS for o in ORDERS] + [("2D-3x2", (4, 3)), ("3D-3x2x2", (5, 4))]
IDS = [f"{z}-Q{o[0]}Q{o[1]}" for z, o in CASES]
X, V, RHO, E, P, CS, DETJ, DIV = slice(0, 3), slice(3, 6), 6, 7, 8, 9, 10, 11


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def set_up(c):
    """Case has a context without the set-up data: lgh_setup_rho0detj0 on the undeformed mesh (what it computes is not used here),
    and the arrays the gauges' masses are formed from: the CURVED mesh of the state and the random density dofs."""
    if getattr(c, "_gauges_ready", False):
        return c
    from laghos_amd import host_lib
    zones = [k for k, v in ZONES.items() if int(np.prod(v)) == c.NE and len(v) == c.dim][0]
    if hasattr(c, "elem_perm"):
        x0 = host_lib.host_disc("cartesian", 0, c.ok, c.ot, 1, zones=ZONES[zones], renumber="random", seed=5)["S0"][:c.dim * c.N]
    else:
        from oracle.fem import Problem
        p = Problem(breaks=[np.linspace(0.0, 1.0, n + 1) for n in ZONES[zones]], order_v=c.ok, order_e=c.ot, problem=1)
        x0 = p.initial_state()[0][:p.H1V]
    NQ = c.ctx.Q1D ** c.dim
    c.ctx.setup_rho0detj0(c.ctx.to_dev(np.ascontiguousarray(x0)), c.rhod, c.ctx.to_dev(np.ones(c.NE * NQ)))
    c.x0 = c.S[:c.dim * c.N].copy()
    c.x0d = c.ctx.to_dev(c.x0)
    c._gauges_ready, c._alone = True, {}
    return c


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(zones_id, order, renumber=None):
        key = (zones_id, tuple(order), renumber)
        if key not in made:
            made[key] = set_up(Case(ZONES[zones_id], order[0], order[1], renumber))
        return made[key]
    yield get
    for c in made.values():
        c.close()


def sample_rows(c, zone, tabs, Sd=None, capacity=1):
    """(rows (n, 12), m_g (n)) of one sample of a set made for it"""
    h = c.ctx.gauges_create(zone, *tabs, c.x0d, c.rhod, capacity)
    try:
        c.ctx.gauges_sample(h, c.Sd if Sd is None else Sd)
        rows = c.ctx.gauges_drain(h)
        assert rows.shape == (1, len(zone), 12)
        return rows[0], c.ctx.gauges_mass(h)
    finally:
        c.ctx.gauges_destroy(h)


def some_gauges(c, n, seed=0, snap=True):
    """n gauges in random zones: random interior xi, and - snap - a third of them with components exactly 0 and 1"""
    rng = np.random.default_rng(100 * c.dim + c.NE + seed)
    zone = rng.integers(0, c.NE, n).astype(np.int32)
    xi = rng.uniform(0.02, 0.98, (n, c.dim))
    if snap:
        for g in range(0, n, 3):
            xi[g, rng.integers(0, c.dim)] = float(rng.integers(0, 2))
        xi[0], xi[n - 1] = 0.0, 1.0        # a corner each
    return zone, xi


def derived_at(c, zone, tabs):
    """detj, div_v and cs of lgh_sample_derived, x, v and e of lgh_sample_fields at the gauges: the two lattice kernels take their
    tables as arguments, so a gauge off every lattice is handed to them as a lattice of its own - its dim table rows as the rows
    of one table (R1 = max(dim, 2)), where point (rx, ry, rz) = (0, 1, 2) of the gauge's zone has the gauge's row on every axis"""
    dim, n = c.dim, len(zone)
    R1 = max(dim, 2)
    NPZ, p = R1 ** dim, sum(a * R1 ** a for a in range(dim))
    NP = c.NE * NPZ
    out = {k: np.zeros((n, dim if k in "xv" else 1)) for k in ("x", "v", "e", "detj", "div_v", "sound_speed")}
    for g in range(n):
        T = [np.ascontiguousarray(np.concatenate([t[g]] * 2)[:R1]) for t in tabs]     # (1D: the row twice)
        dev = {k: c.ctx.to_dev(np.full(a.shape[1] * NP, np.nan)) for k, a in out.items()}
        c.ctx.sample_fields(c.Sd, None, T[0], T[2], x=dev["x"], v=dev["v"], e=dev["e"])
        c.ctx.sample_derived(c.Sd, *T, detj=dev["detj"], div_v=dev["div_v"], sound_speed=dev["sound_speed"])
        c.ctx.sync()
        for k, a in out.items():
            a[g] = dev[k].cpu().numpy().reshape(a.shape[1], NP)[:, zone[g] * NPZ + p]
    return out


def check_exact_relations(c, zone, rows, m, tabs=None):
    g = c.gamma[zone]
    if tabs is not None:   # the bits of the lattice kernels, off the lattice too
        lat = derived_at(c, zone, tabs)
        for k, col in (("sound_speed", CS), ("detj", DETJ), ("div_v", DIV), ("e", E)):
            assert np.array_equal(bits(rows[:, col]), bits(lat[k][:, 0])), k
        assert np.array_equal(bits(rows[:, X][:, :c.dim]), bits(lat["x"])) and np.array_equal(bits(rows[:, V][:, :c.dim]), bits(lat["v"]))
    assert np.array_equal(bits(rows[:, RHO]), bits(m / rows[:, DETJ]))                                    # one IEEE division
    assert np.array_equal(bits(rows[:, P]), bits((g - 1.0) * rows[:, RHO] * np.maximum(rows[:, E], 0.0)))
    want = np.sqrt((g * (g - 1.0)) * np.maximum(rows[:, E], 0.0))
    assert np.all(np.abs(rows[:, CS] - want) <= np.spacing(want))
    assert not rows[:, c.dim:3].any() and not rows[:, 3 + c.dim:6].any()                                  # components >= dim are 0


@pytest.mark.parametrize("zones_id,order", CASES, ids=IDS)
def test_rows_match_numpy(cases, zones_id, order):
    c = cases(zones_id, order)
    zone, xi = some_gauges(c, 13)
    tabs = gr.tables_at(c.ok, c.ot, xi)
    rows, m = sample_rows(c, zone, tabs)
    assert np.all(np.isfinite(rows)) and np.all(np.isfinite(m))
    m_ref, r0 = gr.gauges_mass_reference(c.dim, c.NE, c.N, c.D, c.L, c.h1map, c.x0, c.rho, zone, *tabs)
    ref = gr.gauges_reference(c.dim, c.NE, c.N, c.D, c.L, c.h1map, c.S, c.gamma, zone, *tabs, m)
    H1V = c.dim * c.N
    scale = dict(x=np.abs(c.S[:H1V]).max(), v=np.abs(c.S[H1V:2 * H1V]).max(), e=np.abs(c.S[2 * H1V:]).max())
    for name, col in (("x", X), ("v", V), ("e", E)):
        err = np.abs(rows[:, col] - ref["rows"][:, col]).max()
        print(f"{zones_id} Q{order[0]}Q{order[1]} {name}: max err {err:.3e}, max|field| {scale[name]:.3e}")
        assert err <= TOL * scale[name], name
    ed, el = np.abs(rows[:, DETJ] - ref["rows"][:, DETJ]), np.abs(rows[:, DIV] - ref["rows"][:, DIV])
    print(f"  detj: max err / bound {np.max(ed / (TOL * ref['bound_det'])):.4f}; div_v: {np.max(el / (c.dim * TOL * ref['bound_L'])):.4f}")
    assert np.all(ed <= TOL * ref["bound_det"]) and np.all(el <= c.dim * TOL * ref["bound_L"])
    # m_g = rho0(xi) detJ0(xi): the density to TOL of its largest dof, the determinant to its bound (here x0 is the mesh of S)
    assert np.all(np.abs(m - m_ref) <= TOL * (np.abs(c.rho).max() * np.abs(ref["rows"][:, DETJ]) + np.abs(r0) * ref["bound_det"]) + np.spacing(m_ref))
    check_exact_relations(c, zone, rows, m, tabs)
    neg = rows[:, E] < 0
    assert not rows[neg, P].any() and not rows[neg, CS].any() and np.all(rows[~neg, CS] > 0)
    if c.NE >= 12 and order[1] <= 2:   # the clamp of pressure and sound speed is in play (a Bernstein basis of high order smooths the random e)
        assert neg.any() and not neg.all()
    # with S holding x0, rho is rho0(xi) again: (rho0 det) / det, two roundings.  rho0(xi) in the GPU's own bits: the e column of a
    # state whose e block holds the density dofs
    S2 = np.concatenate([c.x0, c.S[H1V:2 * H1V], c.rho])
    rows2, m2 = sample_rows(c, zone, tabs, Sd=c.ctx.to_dev(S2))
    assert np.array_equal(bits(m2), bits(m))
    eps = np.finfo(np.float64).eps
    assert np.all(np.abs(rows2[:, RHO] - rows2[:, E]) <= 2 * eps * np.abs(rows2[:, E]))
    assert np.array_equal(bits(rows2[:, DETJ]), bits(rows[:, DETJ]))


@pytest.mark.parametrize("zones_id,order", [("1D-257", (3, 2)), ("2D-3x2", (4, 3)), ("3D-3x2x2", (2, 1)), ("3D-5x5x3", (3, 2))])
def test_a_face_point_from_both_zones(cases, zones_id, order):
    """x and v are continuous: the same physical point of a zone face, taken as a gauge of either neighbour, to TOL"""
    c = cases(zones_id, order)
    nz = ZONES[zones_id]
    rng = np.random.default_rng(5)
    zone, xi = [], []
    for a in range(c.dim):
        if nz[a] < 2:
            continue
        for _ in range(3):
            ijk = [int(rng.integers(0, nz[b] - (1 if b == a else 0))) for b in range(c.dim)]
            x = rng.uniform(0, 1, c.dim)
            lo, hi = x.copy(), x.copy()
            lo[a], hi[a] = 1.0, 0.0
            up = list(ijk)
            up[a] += 1
            lex = lambda i: int(sum(i[b] * int(np.prod(nz[:b])) for b in range(c.dim)))
            zone += [lex(ijk), lex(up)]
            xi += [lo, hi]
    assert zone
    rows, _ = sample_rows(c, np.array(zone, dtype=np.int32), gr.tables_at(c.ok, c.ot, np.array(xi)))
    H1V = c.dim * c.N
    for col, s in ((X, np.abs(c.S[:H1V]).max()), (V, np.abs(c.S[H1V:2 * H1V]).max())):
        assert np.abs(rows[0::2, col] - rows[1::2, col]).max() <= TOL * s
    assert np.abs(rows[0::2, E] - rows[1::2, E]).max() > 1e-6     # (e jumps: the pairs are two zones)


LATTICE = [("1D-257", (3, 2)), ("2D-3x2", (4, 3)), ("3D-3x2x2", (2, 1)), ("3D-5x5x3", (3, 2)), ("3D-3x2x2", (5, 4))]


@pytest.mark.parametrize("R1", [2, 9])
@pytest.mark.parametrize("zones_id,order", LATTICE, ids=[f"{z}-Q{o[0]}Q{o[1]}" for z, o in LATTICE])
def test_lattice_gauges_have_the_bits_of_the_dumps(cases, zones_id, order, R1):
    """Gauges at the lattice points r/R of a zone, built from the lattice's own table rows: x, v, e have the bits of
    lgh_sample_fields there, detj, div_v and cs those of lgh_sample_derived."""
    c = cases(zones_id, order)
    dim, z = c.dim, c.NE // 2
    Bh_lat, Gh_lat, Bl_lat = lattice_tables3(c.ok, c.ot, R1 - 1)
    NPZ = R1 ** dim
    r = np.stack([(np.arange(NPZ) // R1 ** a) % R1 for a in range(dim)], axis=1)      # point p = rx + R1 (ry + R1 rz)
    tabs = (Bh_lat[r], Gh_lat[r], Bl_lat[r])                                          # [g, a, :] = row r_a
    rows, _ = sample_rows(c, np.full(NPZ, z, dtype=np.int32), tabs)
    NP = c.NE * NPZ
    out = dict(x=c.ctx.to_dev(np.full(dim * NP, np.nan)), v=c.ctx.to_dev(np.full(dim * NP, np.nan)), e=c.ctx.to_dev(np.full(NP, np.nan)))
    c.ctx.sample_fields(c.Sd, None, Bh_lat, Bl_lat, **out)
    der = dict(detj=c.ctx.to_dev(np.full(NP, np.nan)), div_v=c.ctx.to_dev(np.full(NP, np.nan)), sound_speed=c.ctx.to_dev(np.full(NP, np.nan)))
    c.ctx.sample_derived(c.Sd, Bh_lat, Gh_lat, Bl_lat, **der)
    c.ctx.sync()
    pts = slice(z * NPZ, (z + 1) * NPZ)
    for k, col in (("x", X), ("v", V)):
        assert np.array_equal(bits(rows[:, col][:, :dim].T), bits(out[k].cpu().numpy().reshape(dim, NP)[:, pts])), k
    assert np.array_equal(bits(rows[:, E]), bits(out["e"].cpu().numpy()[pts]))
    for k, col in (("detj", DETJ), ("div_v", DIV), ("sound_speed", CS)):
        assert np.array_equal(bits(rows[:, col]), bits(der[k].cpu().numpy()[pts])), k


def alone(c, z, x):
    """the row of one gauge sampled alone (computed once per gauge)"""
    key = (int(z), tuple(float(v) for v in x))
    if key not in c._alone:
        c._alone[key] = sample_rows(c, np.array([z], dtype=np.int32), gr.tables_at(c.ok, c.ot, np.array([x])))[0][0]
    return c._alone[key]


@pytest.mark.parametrize("zones_id,order", [("1D-257", (2, 1)), ("2D-3x2", (3, 2)), ("3D-5x5x3", (3, 2)), ("3D-3x2x2", (5, 4))])
def test_launch_edges_and_independence(cases, zones_id, order):
    """n around the gauges per workgroup: every row has the bits it has when the gauge is sampled alone, whatever the count, the
    order of the zones and the grid - all gauges in one zone, every gauge in a zone of its own in descending order, a gauge twice"""
    c = cases(zones_id, order)
    probe = c.ctx.gauges_create(np.zeros(1, dtype=np.int32), *gr.tables_at(c.ok, c.ot, np.full((1, c.dim), 0.5)), c.x0d, c.rhod, 1)
    G, groups, lds, threads = c.ctx.gauges_shape(probe)
    c.ctx.gauges_destroy(probe)
    assert 1 <= G <= 4 and groups == 1 and threads == 64 * G and 0 < lds <= 48 * 1024
    rng = np.random.default_rng(9)
    for n in sorted({1, max(G - 1, 1), G, G + 1, 3 * G + 1}):
        xi = rng.uniform(0, 1, (n, c.dim))
        layouts = {"one zone": np.full(n, c.NE - 1), "descending": (c.NE - 1 - np.arange(n)) % c.NE}
        for what, zone in layouts.items():
            zone = zone.astype(np.int32)
            if what == "one zone" and n > 1:
                xi[n - 1] = xi[0]                                  # the same gauge twice
            h = c.ctx.gauges_create(zone, *gr.tables_at(c.ok, c.ot, xi), c.x0d, c.rhod, 1)
            assert c.ctx.gauges_shape(h) == (G, -(-n // G), lds, threads)
            c.ctx.gauges_sample(h, c.Sd)
            rows = c.ctx.gauges_drain(h)[0]
            c.ctx.gauges_destroy(h)
            for g in range(n):
                assert np.array_equal(bits(rows[g]), bits(alone(c, zone[g], xi[g]))), (n, what, g)


def test_buffer_and_drain(cases):
    c = cases("3D-3x2x2", (2, 1))
    zone, xi = some_gauges(c, 5, seed=1)
    tabs = gr.tables_at(c.ok, c.ot, xi)
    rng = np.random.default_rng(2)
    states = [c.S * (1.0 + 0.01 * k) + 1e-3 * rng.uniform(-1, 1, c.S.size) for k in range(5)]
    devs = [c.ctx.to_dev(S) for S in states]
    want = [sample_rows(c, zone, tabs, Sd=d)[0] for d in devs]      # five one-sample sets
    from laghos_amd._lib import LghError
    h = c.ctx.gauges_create(zone, *tabs, c.x0d, c.rhod, 2)
    try:
        assert c.ctx.gauges_pending(h) == 0 and c.ctx.gauges_drain(h).shape == (0, 5, 12)
        got = []
        c.ctx.gauges_sample(h, devs[0])
        assert c.ctx.gauges_pending(h) == 1
        c.ctx.gauges_sample(h, devs[1])
        assert c.ctx.gauges_pending(h) == 2
        with pytest.raises(LghError, match="error 1: .*capacity = 2"):
            c.ctx.gauges_sample(h, devs[2])                          # full: refused, nothing changed
        assert c.ctx.gauges_pending(h) == 2
        got += list(c.ctx.gauges_drain(h))
        assert len(got) == 2 and c.ctx.gauges_pending(h) == 0
        c.ctx.gauges_sample(h, devs[2])
        got += list(c.ctx.gauges_drain(h))                           # a drain of a buffer that is not full
        c.ctx.gauges_sample(h, devs[3])
        c.ctx.gauges_sample(h, devs[4])
        got += list(c.ctx.gauges_drain(h))
        assert c.ctx.gauges_drain(h).shape == (0, 5, 12)
        assert len(got) == 5
        for k in range(5):
            assert np.array_equal(bits(got[k]), bits(want[k])), k    # oldest first
    finally:
        c.ctx.gauges_destroy(h)


def test_nan_dof_shows_in_its_gauges_only(cases):
    c = cases("3D-3x2x2", (2, 1))
    zone = np.arange(c.NE, dtype=np.int32)
    xi = np.random.default_rng(3).uniform(0.1, 0.9, (c.NE, 3))
    tabs = gr.tables_at(c.ok, c.ot, xi)
    good, _ = sample_rows(c, zone, tabs)
    z = 7
    node = int(np.asarray(c.h1map).reshape(c.NE, 27)[z, 13])        # the centre node of a Q2 zone: no other zone holds it
    S = c.S.copy()
    S[c.N + node] = np.nan                                           # its y coordinate
    rows, _ = sample_rows(c, zone, tabs, Sd=c.ctx.to_dev(S))
    others = np.arange(c.NE) != z
    assert np.array_equal(bits(rows[others]), bits(good[others]))
    assert np.isnan(rows[z, 1]) and np.isnan(rows[z, DETJ]) and np.isnan(rows[z, RHO]) and np.isnan(rows[z, DIV])
    assert np.array_equal(bits(rows[z, [0, 2, 3, 4, 5, E, CS]]), bits(good[z, [0, 2, 3, 4, 5, E, CS]]))


def test_inverted_layer_shows_in_its_gauges_only():
    """edge_states' inverted layer of zones on 5 x 2 x 2 zones: detj <= 0 in the gauges of the layer, nothing is trapped, and the
    zones that share no node with the layer keep their bits"""
    from edge_states import edge_state
    from helpers import deformed_state, make_gpu
    from oracle.fem import Problem
    prob = Problem(breaks=[np.linspace(0.0, 1.0, 6), np.linspace(0.0, 1.0, 3), np.linspace(0.0, 1.0, 3)], order_v=2, order_e=1, problem=1)
    g = make_gpu(prob, cg_tol=1e-12)
    try:
        zone = np.arange(prob.NE, dtype=np.int32)
        xi = np.random.default_rng(4).uniform(0.1, 0.9, (prob.NE, 3))
        h = g.gauges(zone, xi, capacity=2)
        g.ctx.gauges_sample(h, g.ctx.to_dev(deformed_state(prob, amp=0.0)))
        g.ctx.gauges_sample(h, g.ctx.to_dev(edge_state(prob, "inverted_layer")))
        plain, inv = g.ctx.gauges_drain(h)
        ix = zone % 5
        assert np.all(inv[ix == 2, DETJ] < 0) and np.all(inv[ix == 2, RHO] < 0) and np.all(plain[:, DETJ] > 0)
        assert np.all(np.isfinite(inv))
        far = (ix == 0) | (ix == 4)
        assert np.array_equal(bits(inv[far]), bits(plain[far]))
        assert np.all(inv[(ix == 1) | (ix == 3), DETJ] > 0)
    finally:
        g.close()


def test_sampling_leaves_the_operator_alone():
    """The quadrature data, its generation counter and the fused force products are untouched: dS/dt of a state is the same bits
    before and after a sample, lgh_quadrature_generation returns the same triple around it, S is unchanged (the test of
    tests/test_gpu_sample.py for the lattice kernel)."""
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
        g.update_quadrature_data(Sd)
        g.ctx.sync()
        triple = g.ctx.quadrature_generation()
        h = g.gauges(np.arange(prob.NE, dtype=np.int32), np.full((prob.NE, 3), 0.25), capacity=4)
        t0 = g.ctx.quadrature_generation()
        g.ctx.gauges_sample(h, Sd)
        g.ctx.sync()
        assert g.ctx.quadrature_generation() == t0 == triple
        assert np.array_equal(Sd.cpu().numpy(), S)
        dS = g.ctx.zeros(S.size)
        g.mult(Sd, dS)                                    # the data the sample must not have touched is used as it stands
        g.ctx.sync()
        assert np.array_equal(dS.cpu().numpy(), before)
        rows = g.ctx.gauges_drain(h)
        assert rows.shape == (1, prob.NE, 12) and np.all(np.isfinite(rows)) and np.all(rows[0, :, DETJ] > 0)
        assert np.array_equal(rhs(), before)
    finally:
        g.close()


def test_rows_sit_at_the_callers_zone_ids(cases):
    """3 x 2 x 2 zones under `-renumber random`: zone j is the structured zone elem_perm[j]; the rows of a gauge given by the caller's
    zone id have the bits the plain mesh gives the same zone for the same state"""
    c, lex = cases("3D-3x2x2", (3, 2), "random"), cases("3D-3x2x2", (3, 2))
    assert not np.array_equal(c.elem_perm, np.arange(c.NE))
    H1V, NL = 3 * c.N, c.L ** 3
    inv = np.argsort(c.elem_perm)                                    # structured zone s is zone inv[s]
    S_lex = np.concatenate([c.S[k * c.N:(k + 1) * c.N][c.node_perm] for k in range(6)] + [c.S[2 * H1V:].reshape(c.NE, NL)[inv].reshape(-1)])
    rho_lex = c.rho.reshape(c.NE, NL)[inv].reshape(-1)
    xi = np.random.default_rng(6).uniform(0, 1, (c.NE, 3))
    tabs = gr.tables_at(c.ok, c.ot, xi)
    zone = np.arange(c.NE, dtype=np.int32)                           # gauge j sits in the caller's zone j
    rows, m = sample_rows(c, zone, tabs)
    # the plain mesh with the same state, masses from the same arrays, gamma of the same zones: a context of its own
    from laghos_amd.context import Context
    from oracle.fem import Problem
    p = Problem(breaks=[np.linspace(0.0, 1.0, n + 1) for n in (3, 2, 2)], order_v=3, order_e=2, problem=1)
    ctx = Context(3, p.NE, c.D, p.B.shape[0], c.L, p.N, np.asarray(p.h1map).reshape(-1), p.B, p.G, p.Bl, p.W, c.gamma[inv], p.ess, order_v=3)
    try:
        ctx.setup_rho0detj0(ctx.to_dev(p.initial_state()[0][:p.H1V]), ctx.to_dev(rho_lex), ctx.to_dev(np.ones(p.NE * p.B.shape[0] ** 3)))
        h = ctx.gauges_create(c.elem_perm[zone].astype(np.int32), *tabs, ctx.to_dev(S_lex[:H1V].copy()), ctx.to_dev(rho_lex), 1)
        ctx.gauges_sample(h, ctx.to_dev(S_lex))
        want, m_lex = ctx.gauges_drain(h)[0], ctx.gauges_mass(h)
    finally:
        ctx.close()
    assert lex.NE == c.NE
    assert np.array_equal(bits(m), bits(m_lex)) and np.array_equal(bits(rows), bits(want))


def rank_gauges(glob, probs, zone_g):
    import rank_cases as rc
    out = []
    for p in probs:
        zm = rc.zone_map(p)
        local = {int(gz): j for j, gz in enumerate(zm)}
        out.append(np.array([local.get(int(z), -1) for z in zone_g], dtype=np.int32))
    return out


def test_two_ranks_drain_the_rows_of_one():
    """2 x 1 emulated ranks (tests/rank_threads.py) with the global state split: the collective drain gives both ranks the same
    bits, and they are the bits of the one-rank rows - signed zeros included: v holds -0.0, and one zone is inverted with e < 0,
    where p = (gamma - 1) (m_g / detj) max(e, 0) is -0.0.  A gauge no rank owns is refused on every rank."""
    import rank_cases as rc
    from helpers import deformed_state, make_gpu
    from laghos_amd._lib import LghError
    from rank_threads import Ranks
    glob, probs = rc.problems((2, 1), "equal", (3, 2))
    S = deformed_state(glob, seed=11, amp=0.05)
    H1V, N, NL = glob.H1V, glob.N, glob.NL
    S[H1V:H1V + N // 2] = -0.0
    hm = np.asarray(glob.h1map).reshape(glob.NE, 4, 4)
    zi = 3 + 26 * 2                                                  # an interior zone of rank 0's block: its interior nodes swap in x
    a, b = hm[zi, 1:3, 1], hm[zi, 1:3, 2]
    S[a], S[b] = S[b].copy(), S[a].copy()
    S[2 * H1V + zi * NL: 2 * H1V + (zi + 1) * NL] = -1.0
    rng = np.random.default_rng(12)
    zone_g = np.concatenate([[zi, zi], rng.integers(0, glob.NE, 9)])
    xi = np.concatenate([[[0.5, 0.5], [0.45, 0.55]], rng.uniform(0, 1, (9, 2))])
    one = make_gpu(glob, cg_tol=1e-12)
    try:
        h = one.gauges(zone_g.astype(np.int32), xi, capacity=2)
        one.ctx.gauges_sample(h, one.ctx.to_dev(S))
        want = one.ctx.gauges_drain(h)[0]
        with pytest.raises(LghError, match="error 1: .*gauge 1 is owned by 0 ranks"):
            one.gauges(np.array([0, -1], dtype=np.int32), xi[:2])
    finally:
        one.close()
    zeros = (want == 0) & np.signbit(want)
    assert want[0, DETJ] < 0 and zeros[:, P].any(), "the state holds no -0.0 to carry"
    zones = rank_gauges(glob, probs, zone_g)
    assert all((z >= 0).any() and (z < 0).any() for z in zones)
    ranks = Ranks(probs, cg_tol=1e-12)
    try:
        def leg(r, op, p):
            hh = op.gauges(zones[r], xi, capacity=2)
            op.ctx.gauges_sample(hh, op.ctx.to_dev(rc.slice_state(p, S)))
            own_m = op.ctx.gauges_mass(hh)
            rows = op.ctx.gauges_drain(hh)[0]
            lost = zones[r].copy()
            lost[4] = -1                                             # gauge 4 on no rank
            try:
                op.gauges(lost, xi)
                refused = ""
            except LghError as ex:
                refused = str(ex)
            return rows, own_m, refused
        got = ranks.run(leg)
    finally:
        ranks.close()
    for r in range(2):
        assert np.array_equal(bits(got[r][0]), bits(want)), r
        assert "gauge 4 is owned by 0 ranks" in got[r][2], got[r][2]
        mine = zones[r] >= 0
        assert np.all(np.signbit(got[r][1][~mine]) & (got[r][1][~mine] == 0)) and np.all(got[r][1][mine] != 0)


def test_refusals(cases):
    from laghos_amd._lib import LghError
    c = cases("2D-3x2", (2, 1))
    zone, xi = some_gauges(c, 4, snap=False)
    Bh, Gh, Bl = gr.tables_at(c.ok, c.ot, xi)
    ok = lambda **kw: c.ctx.gauges_create(kw.get("zone", zone), kw.get("Bh", Bh), kw.get("Gh", Gh), kw.get("Bl", Bl), c.x0d, c.rhod, kw.get("capacity", 4))
    with pytest.raises(LghError, match="error 1: .*capacity = 0"):
        ok(capacity=0)
    with pytest.raises(LghError, match="error 1: .*n = 0"):
        c.ctx.gauges_create(np.zeros(0, np.int32), np.zeros(0), np.zeros(0), np.zeros(0), c.x0d, c.rhod, 4)
    for bad in (-2, c.NE):
        z = zone.copy()
        z[2] = bad
        with pytest.raises(LghError, match=rf"error 1: .*zone\[2\] = {bad} "):
            ok(zone=z)
    z = zone.copy()
    z[1] = -1
    with pytest.raises(LghError, match="error 1: .*gauge 1 is owned by 0 ranks"):
        ok(zone=z)
    for name, T in (("Bh", Bh), ("Gh", Gh), ("Bl", Bl)):
        for v in (np.nan, np.inf):
            T2 = T.copy()
            T2[3, 1, 0] = v
            with pytest.raises(LghError, match=rf"error 1: .*{name}\[.*not finite \(gauge 3\)"):
                ok(**{name: T2})
    # NULL arguments, straight at the library
    L, h = c.ctx.lib, ctypes.c_int(-1)
    z, tabs = np.ascontiguousarray(zone, dtype=np.int32), [np.ascontiguousarray(T.reshape(-1)) for T in (Bh, Gh, Bl)]
    args = [z.ctypes.data_as(ctypes.POINTER(ctypes.c_int))] + [T.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) for T in tabs] + \
           [ctypes.c_void_p(c.x0d.data_ptr()), ctypes.c_void_p(c.rhod.data_ptr())]
    for k, name in enumerate(("zone", "Bh", "Gh", "Bl", "x0_h1", "rho0_l2")):
        a = list(args)
        a[k] = None
        assert L.lgh_gauges_create(c.ctx.h, 4, *a, 4, ctypes.byref(h)) == 1 and f"{name} is NULL".encode() in L.lgh_last_error()
    assert L.lgh_gauges_create(c.ctx.h, 4, *args, 4, None) == 1 and b"handle is NULL" in L.lgh_last_error()
    good = ok()
    assert L.lgh_gauges_sample(c.ctx.h, good, None) == 1 and b"S is NULL" in L.lgh_last_error()
    for call in (lambda: c.ctx.gauges_sample(good + 7, c.Sd), lambda: c.ctx.gauges_pending(-1), lambda: c.ctx.gauges_drain(good + 7),
                 lambda: c.ctx.gauges_mass(99), lambda: c.ctx.gauges_shape(99), lambda: c.ctx.gauges_destroy(99)):
        with pytest.raises(LghError, match="error 1: .*handle .* names no gauge set"):
            call()
    # the context stays usable, and nothing was kept of the refused sets: the next handle is the next one
    c.ctx.gauges_sample(good, c.Sd)
    rows = c.ctx.gauges_drain(good)
    assert rows.shape == (1, 4, 12) and np.all(np.isfinite(rows))
    c.ctx.gauges_destroy(good)
    with pytest.raises(LghError, match="names no gauge set"):
        c.ctx.gauges_sample(good, c.Sd)
    assert ok() == good                                              # the slot is free again
    c.ctx.gauges_destroy(good)


def test_refused_before_the_set_up():
    from laghos_amd._lib import LghError
    c = Case(ZONES["2D-3x2"], 2, 1)
    try:
        xi = np.full((1, 2), 0.5)
        with pytest.raises(LghError, match="error 1: .*lgh_setup_rho0detj0"):
            c.ctx.gauges_create(np.zeros(1, np.int32), *gr.tables_at(2, 1, xi), c.ctx.to_dev(c.S[:2 * c.N].copy()), c.rhod, 4)
        set_up(c)
        h = c.ctx.gauges_create(np.zeros(1, np.int32), *gr.tables_at(2, 1, xi), c.x0d, c.rhod, 4)
        c.ctx.gauges_sample(h, c.Sd)
        assert np.all(np.isfinite(c.ctx.gauges_drain(h)))
    finally:
        c.close()


def test_ktime_times_a_sample(cases):
    c = cases("3D-5x5x3", (3, 2))
    zone, xi = some_gauges(c, 64)
    h = c.ctx.gauges_create(zone, *gr.tables_at(c.ok, c.ot, xi), c.x0d, c.rhod, 8)
    try:
        L = c.ctx.lib
        assert L.lgh_ktime_begin(c.ctx.h, 18, 8) == 0                # LGH_KERNEL_GAUGES
        for _ in range(5):
            c.ctx.gauges_sample(h, c.Sd)
        n, mean = ctypes.c_int(-1), ctypes.c_double(-1.0)
        assert L.lgh_ktime_end(c.ctx.h, ctypes.byref(n), ctypes.byref(mean)) == 0
        print(f"lgh_gauges_sample, 64 gauges on 5x5x3 Q3Q2: {mean.value * 1e6:.1f} us per sample")
        assert n.value == 5 and 0.0 < mean.value < 1e-2
        assert len(c.ctx.gauges_drain(h)) == 5
    finally:
        c.ctx.gauges_destroy(h)
