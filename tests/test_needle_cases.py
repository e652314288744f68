"""The needles of tests/needle_cases.py on the oracle alone (no GPU): what tests/test_gpu_fast_path_checks.py takes for
granted is checked here, where a failure says "the case is wrong", not "the check is wrong".  These are conditions, not
measurements: an input that misses one is replaced, the condition stays.

  * visible   for every needle that is meant to show in the numbers, the WRONG fast path is emulated in the oracle (the
              compact table W[q] mean(D / W) in place of the needled one; every point's Jac0inv replaced by the zone's
              first; half a table mirrored; the weights rebuilt from their first row; F.1 for F.x; F^T v_old for F^T v)
              and differs from the oracle's right answer by at least 100 x the bar the GPU result is held to, in the
              same max-norm rel_err;
  * local     a needle changes the oracle's answer only in dofs of the zones it touches - bit for bit elsewhere;
  * clear of the thresholds   on every mesh that carries a threshold needle (Q2Q1, Q3Q2, Q4Q3; Q1Q0 and 2D meet it too)
              the spread a check looks at (needle_cases.mass_spread, jac0_spread) is <= 1e-13 in every untouched zone,
              <= 2.5e-13 for every "just below" needle and >= 4e-12 for every "just above" one (the checks admit 1e-12).
              The 1e-13 covers the threshold meshes ONLY: the Q5Q4 mesh (17x1x1, set by the issue; tables and weights
              alone are needled there) reaches 1.1e-13 at the far end of its row, whatever its length - x / h is 17 there
              - and is held to the 2.5e-13 of a "just below" needle: what matters on it is that the checks say "compact";
  * one point alone   the small mass needle and the corner-vertex needle put exactly ONE point of a zone beyond what the
              check admits and leave every other point of the zone, and every other zone, within it;
  * conditioned   the 1-D mass tiles of every skewed or needled table stay within a factor 2 of the symmetric ones in
              condition number, so the project's bars apply unchanged; every skewed or needled weight is positive and a
              SkewRule table is asymmetric by >= 1e-3.

Measured: one mass entry x 1.5 moves the H1 mass product by 1.6e-4 to 2.6e-3 of its largest entry (27 or 64 of 3003 /
9424 nodes); a bubble node moved by 0.1 h gives a Jac0inv spread of 0.145 to 0.18 in its zone and <= 4.7e-14 in every
other, by 1e-10 h 1.5e-10 to 2.2e-10, by 1e-14 h 1.4e-14 to 2.3e-14; base spreads of the mass data <= 4.1e-14."""
import ctypes

import numpy as np
import pytest

import needle_cases as nc
from helpers import deformed_state, make_oracle, rel_err, seeded

ORDERS_3D = [(1, 0), (2, 1), (3, 2), (4, 3), (5, 4)]
NEEDLE_ORDERS = [(2, 1), (3, 2)]          # the 300-zone mesh
CURVED_ORDERS = [(2, 1), (3, 2), (4, 3)]
ALL = [(3, o) for o in ORDERS_3D] + [(2, o) for o in nc.ORDERS_2D]
oid = lambda o: f"Q{o[0]}Q{o[1]}"
did = lambda c: f"{c[0]}D-Q{c[1][0]}Q{c[1][1]}"


_BASES = {}


def _base(order, dim=3):
    """(problem, oracle, its mass table, its mass products of seeded vectors): shared, never left modified; closed by the
    module's fixture below"""
    if (order, dim) not in _BASES:
        prob = nc.problem(order, dim=dim)
        o = make_oracle(prob)
        xv, xe = seeded(prob.N, 21), seeded(prob.L2V, 22)
        _BASES[(order, dim)] = (prob, o, o.massD.copy(), (xv, xe, o.mass_mult(0, xv), o.mass_mult(1, xe)))
    return _BASES[(order, dim)]


@pytest.fixture(scope="module", autouse=True)
def _close_shared_oracles():
    yield
    while _BASES:
        _BASES.popitem()[1][1].close()


def _zone_nodes(prob, zones):
    return np.unique(np.asarray(prob.h1map).reshape(prob.NE, prob.ND)[np.atleast_1d(zones)])


def _zone_l2(prob, zones):
    return (np.atleast_1d(zones)[:, None] * prob.NL + np.arange(prob.NL)[None, :]).reshape(-1)


def _only_in(a, b, idx):
    """a and b have the same bits outside idx"""
    m = np.ones(a.size, dtype=bool)
    m[idx] = False
    return np.array_equal(a[m], b[m])


# ---- the meshes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL, ids=did)
def test_base_spreads(case):
    """every mesh of the needle cases is affine zone by zone, far inside what the checks admit"""
    dim, order = case
    prob, o, D0, _ = _base(order, dim)
    ms, _ = nc.mass_spread(D0, prob.W, prob.NE)
    js, _ = nc.jac0_spread(o.Jac0inv, prob.NE, prob.NQ, dim * dim)
    print(f"{did(case)}: NE {prob.NE} N {prob.N} mass spread {ms.max():.2e} Jac0inv spread {js.max():.2e}")
    # (<= 1e-13 on every mesh that carries a threshold needle; Q5Q4 carries none - see the module docstring)
    bound = nc.SPREAD_BELOW if order == (5, 4) else nc.SPREAD_BASE
    assert ms.max() <= bound and js.max() <= bound
    if order in NEEDLE_ORDERS and dim == 3:
        assert prob.NE == 300 and prob.NE % 256 == 44 and prob.NE % 64 == 44
    # the parities the three code paths of vec_differs_k hang on: v = S + H1V is 16-byte aligned when H1V is even
    if case == (3, (2, 1)):
        assert prob.H1V % 2 == 1
    if case == (3, (3, 2)):
        assert prob.H1V % 2 == 0


# ---- A: one entry of the mass table --------------------------------------------------------------------------------------
MASS_CASES = [(o, i) for o in NEEDLE_ORDERS for i in range(5)]


@pytest.mark.parametrize("order,i", MASS_CASES, ids=[f"{oid(o)}-pos{i}" for o, i in MASS_CASES])
def test_mass_needle_is_visible_and_local(order, i):
    prob, o, D0, (xv, xe, yv0, ye0) = _base(order)
    z, q = nc.zone_points(prob.NE, prob.NQ)[i]
    Dn = D0.copy()
    Dn[z * prob.NQ + q] *= 1.5
    spread, compact = nc.mass_spread(Dn, prob.W, prob.NE)
    try:
        o.massD[:] = Dn
        yv, ye = o.mass_mult(0, xv), o.mass_mult(1, xe)
        o.massD[:] = compact                      # what the kernels would read had the check said "compact"
        yv_w, ye_w = o.mass_mult(0, xv), o.mass_mult(1, xe)
    finally:
        o.massD[:] = D0
    print(f"{oid(order)} ({z}, {q}): spread {spread[z]:.2e}; wrong path off by {rel_err(yv_w, yv):.2e} (H1) {rel_err(ye_w, ye):.2e} (L2);"
          f" {int(np.sum(yv != yv0))} of {prob.N} nodes change")
    assert spread[z] > 0.1 and np.delete(spread, z).max() <= nc.SPREAD_BASE
    assert rel_err(yv_w, yv) >= 100 * nc.BAR_STORED and rel_err(ye_w, ye) >= 100 * nc.BAR_STORED
    assert _only_in(yv, yv0, _zone_nodes(prob, z)) and _only_in(ye, ye0, _zone_l2(prob, z))
    assert np.any(yv != yv0) and np.any(ye != ye0)


@pytest.mark.parametrize("order,i", MASS_CASES, ids=[f"{oid(o)}-pos{i}" for o, i in MASS_CASES])
def test_small_mass_needle_shows_at_its_own_point_only(order, i):
    """A factor 1.5 moves the zone's mean of D / W so far that EVERY point of the zone is off: a check that skipped the
    needled point would still say "stored".  1 + 3e-11 is thirty times what the check admits at its own point and moves the
    others by 3e-11 / NQ, less than half of it: only a check that looks at this very point sees it."""
    prob, o, D0, _ = _base(order)
    z, q = nc.zone_points(prob.NE, prob.NQ)[i]
    Dn = D0.copy()
    Dn[z * prob.NQ + q] *= nc.MASS_SMALL
    De = Dn.reshape(prob.NE, prob.NQ)[z]
    s = np.mean(De / prob.W)
    dev = np.abs(De - prob.W * s) / np.abs(De)
    print(f"{oid(order)} ({z}, {q}): the needle {dev[q]:.2e}, the zone's other points <= {np.delete(dev, q).max():.2e}")
    assert dev[q] >= nc.SPREAD_ABOVE and np.delete(dev, q).max() <= 0.5 * nc.CHECK_TOL
    assert np.delete(nc.mass_spread(Dn, prob.W, prob.NE)[0], z).max() <= nc.SPREAD_BASE


def test_mass_threshold_needles_are_clear_of_rounding():
    prob, o, D0, _ = _base((3, 2))
    k = nc.mass_threshold_position(D0, prob.W, prob.NE)
    z = k // prob.NQ
    for factor, above in ((nc.MASS_ABOVE, True), (nc.MASS_BELOW, False)):
        Dn = D0.copy()
        Dn[k] *= factor
        spread, _ = nc.mass_spread(Dn, prob.W, prob.NE)
        print(f"factor 1 + {factor - 1:.1e} at entry {k} (zone {z}): spread {spread[z]:.3e}, elsewhere {np.delete(spread, z).max():.2e}")
        assert np.delete(spread, z).max() <= nc.SPREAD_BASE
        assert spread[z] >= nc.SPREAD_ABOVE if above else spread.max() <= nc.SPREAD_BELOW


# ---- B: one curved zone ----------------------------------------------------------------------------------------------------
CURVED_CASES = [(o, i) for o in CURVED_ORDERS + [(1, 0)] for i in range(len(nc.curved_zones(int(np.prod(nc.MESH_3D[o])))))]


@pytest.mark.parametrize("order,i", CURVED_CASES, ids=[f"{oid(o)}-zone{i}" for o, i in CURVED_CASES])
def test_one_curved_zone_is_visible_and_local(order, i):
    base, o0, _, _ = _base(order)
    zone = nc.curved_zones(base.NE)[i]
    prob = nc.OneCurvedZone(base, zone, 0.1)
    assert len(prob.touched) == (1 if order[0] >= 2 else 2 if zone < base.NE - 1 else 1)
    NE, NQ, n2 = base.NE, base.NQ, 9
    S0, S = deformed_state(base), deformed_state(prob)
    assert np.sum(S0 != S) == 3                                   # the three coordinates of one node
    o = make_oracle(prob)
    try:
        ms, _ = nc.mass_spread(o.massD, base.W, NE)
        js, first = nc.jac0_spread(o.Jac0inv, NE, NQ, n2)
        other = np.ones(NE, dtype=bool)
        other[prob.touched] = False
        assert js[prob.touched].min() > 0.01 and ms[prob.touched].min() > 0.01
        assert js[other].max() <= nc.SPREAD_BASE and ms[other].max() <= nc.SPREAD_BASE
        # (the length scale of the viscosity comes from the volume of the whole mesh, which the moved node changes: with the
        #  base mesh's h0 what is left of the needle is what its zone sees)
        o.L.lgo_set_h0(o.h, ctypes.c_double(o0.h0))
        o.reset_time_step_estimate()
        o.update_quadrature_data(S)
        sj = o.stressJinvT.copy()
        o.Jac0inv[:] = first                                      # what the update would read had the check said "compact"
        o.qdata_is_current = False
        o.update_quadrature_data(S)
        sj_w = o.stressJinvT.copy()
    finally:
        o.close()
    o0.reset_time_step_estimate()
    o0.qdata_is_current = False
    o0.update_quadrature_data(S0)
    sj0 = o0.stressJinvT.copy()
    print(f"{oid(order)} zone {zone}: Jac0inv spread {js[prob.touched].min():.3f} (elsewhere {js[other].max():.1e}),"
          f" wrong path off by {rel_err(sj_w, sj):.2e} in stressJinvT")
    assert rel_err(sj_w, sj) >= 100 * nc.BAR_QDATA
    # (stressJinvT[q + NQ (e + NE k)]: nine planes of NE * NQ)
    rows = (np.arange(n2)[:, None, None] * NE * NQ + prob.touched[None, :, None] * NQ + np.arange(NQ)[None, None, :]).reshape(-1)
    assert _only_in(sj, sj0, rows) and np.any(sj != sj0)


@pytest.mark.parametrize("order", CURVED_ORDERS, ids=oid)
def test_curved_threshold_needles_are_clear_of_rounding(order):
    base = _base(order)[0]
    for zone in nc.curved_zones(base.NE):
        for delta, above in ((nc.CURVE_ABOVE, True), (nc.CURVE_BELOW, False)):
            o = make_oracle(nc.OneCurvedZone(base, zone, delta))
            try:
                js, _ = nc.jac0_spread(o.Jac0inv, base.NE, base.NQ, 9)
            finally:
                o.close()
            print(f"{oid(order)} zone {zone} delta {delta:.0e}: spread {js[zone]:.2e}, elsewhere {np.delete(js, zone).max():.1e}")
            assert np.delete(js, zone).max() <= nc.SPREAD_BASE
            assert js[zone] >= nc.SPREAD_ABOVE if above else js.max() <= nc.SPREAD_BELOW


@pytest.mark.parametrize("order", sorted(nc.CORNER_DELTA), ids=oid)
def test_corner_vertex_needle_shows_at_the_last_point_only(order):
    """A moved bubble node deviates at every point of its zone: a check that skipped one point would still say "stored".
    The far corner vertex of the last zone, moved by CORNER_DELTA, takes Jac0inv beyond the 1e-12 of the check at the
    zone's LAST point alone (the nearest to that vertex); every other point stays within 0.85e-12, every other zone
    within 1e-13 - and the rounding of the values themselves (<= 5e-14) is far inside both margins."""
    base = _base(order)[0]
    zone = base.NE - 1
    prob = nc.OneCurvedZone(base, zone, nc.CORNER_DELTA[order], vertex=True)
    assert list(prob.touched) == [zone]
    o = make_oracle(prob)
    try:
        dev = nc.jac0_point_spread(o.Jac0inv, base.NE, base.NQ, 9)
    finally:
        o.close()
    d = dev[zone]
    print(f"{oid(order)}: the last point {d[-1]:.3e}, the zone's other points <= {d[:-1].max():.3e}, other zones <= {np.delete(dev, zone, axis=0).max():.1e}")
    assert d[-1] >= nc.CORNER_LAST > nc.CHECK_TOL > nc.CORNER_OTHERS >= d[:-1].max()
    assert np.delete(dev, zone, axis=0).max() <= nc.SPREAD_BASE


# ---- C, D: tables and weights ------------------------------------------------------------------------------------------------
def _mass_products(prob):
    o = make_oracle(prob)
    try:
        return o.mass_mult(0, seeded(prob.N, 21)), o.mass_mult(1, seeded(prob.L2V, 22))
    finally:
        o.close()


def _well_conditioned(prob, base):
    """positive weights; 1-D mass tiles within a factor 2 of the symmetric rule's in condition number"""
    assert np.all(np.asarray(prob.W) > 0)
    w, w0 = np.asarray(prob.W)[:prob.Q1D] / np.asarray(prob.W)[0] * prob.qwts[0], np.asarray(base.qwts)
    for T, T0 in ((prob.B, base.B), (prob.Bl, base.Bl)):
        c, c0 = nc.tile_condition(T, w), nc.tile_condition(T0, w0)
        assert 0.5 * c0 <= c <= 2.0 * c0, (c, c0)


def _asymmetry(T):
    flat = np.asarray(T).T.reshape(-1)
    return float(np.abs(flat - flat[::-1]).max())


@pytest.mark.parametrize("case", ALL, ids=did)
def test_skew_rule(case):
    """SkewRule(0.1, 0.3): asymmetric tables and weights, well conditioned, the mass data still W[q] s_e and the zones
    affine; a kernel that mirrored half a table, or rebuilt the weights from half of them, is off by >= 100 bars"""
    dim, order = case
    base = _base(order, dim)[0]
    prob = nc.SkewRule(base, 0.1, 0.3)
    _well_conditioned(prob, base)
    print(f"{did(case)}: asymmetry of B {_asymmetry(prob.B):.3f} Bl {_asymmetry(prob.Bl):.3f}")
    assert _asymmetry(prob.B) >= 1e-3
    assert order[1] == 0 or _asymmetry(prob.Bl) >= 1e-3           # (the Bernstein basis of order 0 is the constant 1)
    assert _asymmetry(base.B) <= 1e-14 and _asymmetry(base.Bl) <= 1e-14
    o = make_oracle(prob)
    try:
        ms, _ = nc.mass_spread(o.massD, prob.W, prob.NE)
        js, _ = nc.jac0_spread(o.Jac0inv, prob.NE, prob.NQ, dim * dim)
        bound = nc.SPREAD_BELOW if order == (5, 4) else nc.SPREAD_BASE     # (as test_base_spreads)
        assert ms.max() <= bound and js.max() <= bound
    finally:
        o.close()
    yv, ye = _mass_products(prob)
    for keep in (0, 1):
        yv_w, ye_w = _mass_products(nc.WithTables(prob, B=nc.mirrored(prob.B, keep), Bl=nc.mirrored(prob.Bl, keep)))
        assert rel_err(yv_w, yv) >= 100 * nc.BAR_COMPACT
        assert order[1] == 0 or rel_err(ye_w, ye) >= 100 * nc.BAR_COMPACT
    yv_w, ye_w = _mass_products(nc.WithTables(prob, W=nc.rebuilt_weights(prob.W, prob.Q1D, dim)))
    assert rel_err(yv_w, yv) >= 100 * nc.BAR_COMPACT and rel_err(ye_w, ye) >= 100 * nc.BAR_COMPACT


@pytest.mark.parametrize("order", ORDERS_3D[1:], ids=oid)
def test_skewed_weights_alone(order):
    """SkewRule(0, 0.3): symmetric tables, a tensor product of asymmetric 1-D weights"""
    base = _base(order)[0]
    prob = nc.SkewRule(base, 0.0, 0.3)
    _well_conditioned(prob, base)
    assert np.array_equal(prob.B, base.B) and np.array_equal(prob.Bl, base.Bl)
    w = prob.qwts
    assert np.abs(w - w[::-1]).max() >= 1e-3 * w.max()
    yv, ye = _mass_products(prob)
    yv_w, ye_w = _mass_products(nc.WithTables(prob, W=nc.rebuilt_weights(prob.W, prob.Q1D, 3)))
    print(f"{oid(order)}: weights mirrored from their first half: off by {rel_err(yv_w, yv):.2e} (H1) {rel_err(ye_w, ye):.2e} (L2)")
    assert rel_err(yv_w, yv) >= 100 * nc.BAR_COMPACT and rel_err(ye_w, ye) >= 100 * nc.BAR_COMPACT


TABLE_CASES = [(o, w, i) for o in NEEDLE_ORDERS for w in ("B", "Bl") for i in range(3)]


@pytest.mark.parametrize("order,which,i", TABLE_CASES, ids=[f"{oid(o)}-{w}-{i}" for o, w, i in TABLE_CASES])
def test_table_needle(order, which, i):
    """1e-6 on one entry of B or Bl: a kernel that keeps half the table (either half) is off by >= 100 bars in the mass
    operator of that space"""
    base = _base(order)[0]
    n = base.Q1D * (base.D1D if which == "B" else base.L1D)
    prob = nc.TableNeedle(base, which, nc.table_indices(n)[i], eps=1e-6)
    _well_conditioned(prob, base)
    assert 0.9e-6 <= _asymmetry(getattr(prob, which)) <= 1.1e-6
    # B enters the geometry: with one entry off the basis no longer sums to 1 at that point, the Jacobian - and with it the
    # mass data - varies inside EVERY zone, far beyond what the checks admit; Bl does not: both stay compact
    o = make_oracle(prob)
    try:
        ms, js = nc.mass_spread(o.massD, prob.W, prob.NE)[0], nc.jac0_spread(o.Jac0inv, prob.NE, prob.NQ, 9)[0]
    finally:
        o.close()
    if which == "B":
        assert ms.min() >= 1e3 * nc.SPREAD_ABOVE and js.min() >= 1e3 * nc.SPREAD_ABOVE
    else:
        assert ms.max() <= nc.SPREAD_BASE and js.max() <= nc.SPREAD_BASE
    space = 0 if which == "B" else 1
    y = _mass_products(prob)[space]
    errs = [rel_err(_mass_products(nc.WithTables(prob, **{which: nc.mirrored(getattr(prob, which), keep)}))[space], y) for keep in (0, 1)]
    print(f"{oid(order)} {which}[{prob.index}]: half a table mirrored: off by {errs[0]:.2e} / {errs[1]:.2e}")
    assert min(errs) >= 100 * nc.BAR_COMPACT


WEIGHT_CASES = [(o, i) for o in ORDERS_3D[1:] for i in range(3)]


@pytest.mark.parametrize("order,i", WEIGHT_CASES, ids=[f"{oid(o)}-{i}" for o, i in WEIGHT_CASES])
def test_weight_needle(order, i):
    """one weight x (1 + 1e-6): no tensor product any more; weights rebuilt from the first row are off by >= 100 bars.  The
    same entry x (1 + 2^-46) is beyond what the check admits (1.8e-15) by a factor 8 - a report, nothing to see in numbers"""
    base = _base(order)[0]
    q = nc.table_indices(base.NQ)[i]
    prob = nc.TableNeedle(base, "W", q, scale=1.0 + 1e-6)
    assert np.all(prob.W > 0)
    # the 1-D mass tiles on the row of weights that holds the needle (the scale of a row does not enter a condition number)
    Q = base.Q1D
    row = prob.W.reshape(Q, Q, Q)[q // (Q * Q), (q // Q) % Q, :]
    assert row[q % Q] == prob.W[q]
    for T in (base.B, base.Bl):
        c, c0 = nc.tile_condition(T, row), nc.tile_condition(T, base.qwts)
        assert 0.5 * c0 <= c <= 2.0 * c0, (c, c0)
    yv, ye = _mass_products(prob)
    Wr = nc.rebuilt_weights(prob.W, base.Q1D, 3)
    yv_w, ye_w = _mass_products(nc.WithTables(prob, W=Wr))
    print(f"{oid(order)} W[{q}]: rebuilt weights off by {np.abs(Wr / prob.W - 1).max():.2e}; products {rel_err(yv_w, yv):.2e} (H1) {rel_err(ye_w, ye):.2e} (L2)")
    assert rel_err(yv_w, yv) >= 100 * nc.BAR_COMPACT and rel_err(ye_w, ye) >= 100 * nc.BAR_COMPACT
    tiny = nc.TableNeedle(base, "W", q, scale=1.0 + 2.0 ** -46)
    assert np.abs(nc.rebuilt_weights(tiny.W, base.Q1D, 3) / tiny.W - 1).max() >= 4 * 1.8e-15
    # the rule of the generator itself passes the check: rebuilt weights within the 1.8e-15 it admits
    assert np.abs(nc.rebuilt_weights(base.W, base.Q1D, 3) / base.W - 1).max() <= 1.8e-15


# ---- E, F: the vectors ---------------------------------------------------------------------------------------------------------
def _stress_state(order):
    prob, o, _, _ = _base(order)
    S = deformed_state(prob)
    o.reset_time_step_estimate()
    o.qdata_is_current = False
    o.update_quadrature_data(S)
    return prob, o, S


@pytest.mark.parametrize("order", NEEDLE_ORDERS, ids=oid)
def test_velocity_needles_are_visible_and_local(order):
    """one entry of v changed by 50 %: F^T v_old in place of F^T v is off by >= 100 bars, in the zones of that node only"""
    prob, o, S = _stress_state(order)
    H1V, N = prob.H1V, prob.N
    v = S[H1V:2 * H1V].copy()
    ref = o.force_mult_transpose(v)
    hm = np.asarray(prob.h1map).reshape(prob.NE, prob.ND)
    for k in nc.vector_indices(H1V):
        vn = v.copy()
        vn[k] *= 1.5
        y = o.force_mult_transpose(vn)
        zones = np.nonzero((hm == k % N).any(axis=1))[0]
        print(f"{oid(order)} v[{k}]: F^T v_old off by {rel_err(ref, y):.2e}, {len(zones)} zone(s)")
        assert rel_err(ref, y) >= 100 * nc.BAR_QDATA
        assert _only_in(y, ref, _zone_l2(prob, zones))


def one_indices(L2V):
    return [0, 257 + 13, L2V - 1]


@pytest.mark.parametrize("order", NEEDLE_ORDERS, ids=oid)
def test_one_needles_are_visible(order):
    """x = 1 except one entry 0.5: F.1 in place of F.x is off by >= 100 bars on the rows that are compared (the rows of a
    component that are not essential for it)"""
    prob, o, S = _stress_state(order)
    F1 = o.force_mult(np.ones(prob.L2V))
    free = np.ones(prob.H1V, dtype=bool)
    for c in range(3):
        free[c * prob.N + np.asarray(prob.ess[c], dtype=np.int64)] = False
    assert prob.L2V > 512
    for k in one_indices(prob.L2V):
        x = np.ones(prob.L2V)
        x[k] = 0.5
        Fx = o.force_mult(x)
        print(f"{oid(order)} x[{k}]: F.1 off by {rel_err(F1[free], Fx[free]):.2e}")
        assert rel_err(F1[free], Fx[free]) >= 100 * nc.BAR_QDATA
        assert _only_in(Fx, F1, np.concatenate([c * prob.N + _zone_nodes(prob, k // prob.NL) for c in range(3)]))
