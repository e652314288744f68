"""Every check that selects a fast path from the caller's data, with ONE deviating entry (tests/needle_cases.py; the
conditions these tests rely on are proved on the oracle alone in tests/test_needle_cases.py).

The library takes a fast path where it finds a property in the data; the fast kernel is then only as correct as the
check.  Every other test has the checks pass everywhere (Cartesian meshes, the generator's tables), fail everywhere
(every entry scaled, every node moved) or bypassed by a switch.  Here:

  A  one entry of the mass table (mass_rank1_k: compact data W[q] s_e, the Kronecker K1, the slab K1's Kronecker pass, the
     L2 Kronecker apply and its fused update), through both write routes, at the edges of the check's 256-zone workgroups
     of a 300-zone mesh; values 0, -|D|, +inf and NaN; factors just across the 1e-12 of the check
  B  one curved zone (jac0_compact_k, 64 zones per workgroup: one Jac0inv per zone in the row-form update), at zones 0, 63,
     64 and the last; node shifts just across the 1e-12 of the check; a corner vertex that bends the last point alone
  C  asymmetric tables (the `mirror` loop of lgh_create: half a table in scalar registers): a skewed rule at every order,
     3D and 2D, and one entry of B or of Bl off by 1e-6 / 1e-13
  D  weights that are no symmetric tensor product (the weights loop of lgh_create: weights from Q / 2 scalars, the 1-D mass
     tiles, every Kronecker form): one entry x (1 + 1e-6), x (1 + 2^-46), and asymmetric 1-D weights under symmetric tables
  E  "the velocity of the state" (vec_differs_k: 16-byte loads, the odd tail, the scalar path of an unaligned vector, the
     strided grid above 2 * 2048 * 256 entries): one entry changed by 50 %, by one ulp, to -0.0, to NaN
  F  "the constant one" (not_all_ones_k): one entry 0.5

Bars are the project's: operators 1e-13 of the largest entry against the stored table and 2e-12 against compact data,
stressJinvT and dt 1e-12, force products 1e-12, dx/dt 1e-13, dv/dt and de/dt 1e-10 with both CGs at 1e-14 (de/dt 1e-8 at
Q5Q4; tests/test_gpu_shapes_solve.py), 1e-9 with the CGs at 1e-13 on a curved mesh (test_rhs_on_a_curved_initial_mesh_vs_oracle),
CG solutions 1e-8.  Contexts are shared per configuration (the `boxes` fixture); the mass needles go in and out through
the writable pointers.

Neither write route of the mass table is the whole contract alone: calling lgh_mass_D() again has the form looked for
again, lgh_mass_data_changed() reassembles the Jacobi diagonal as well.  K1 is therefore compared with d formed from the
DEVICE's diagonal, and the diagonal itself is held to the oracle's operator after lgh_mass_data_changed().

Findings.  No check missed a needle and no result was off.  Three expectations had to be put right, each in the TEST:
  * one entry of B off by 1e-6 breaks the partition of unity at that point, so the Jacobian - and with it the mass data
    - varies inside every zone by 2e-6 / 5e-6: the stored table and the point values of Jac0inv are what the checks must
    find there (and do); the expected forms now come from the oracle's arrays (found_compact);
  * lgh_mass_D() called again does not reassemble the Jacobi diagonal (include/laghos_hip.h says so): a table restored
    through it after lgh_mass_data_changed() had seen the needle leaves the needle's diagonal behind - the same operator,
    other bits of K1's d = r / diag;
  * the ORACLE's volume is a running sum over NE * NQ points and is off by up to 1.1e-13 from the exact sum of the same
    points on the equal Q4Q3 mesh (the device's by at most 1.3e-15): the volume is held to math.fsum of the oracle's points.
A needle that moves a whole zone - a factor 1.5 on one mass entry shifts the zone's mean, a moved bubble node bends every
point - is seen at EVERY point of the zone, so a check that skipped one point would still report it.  Two needles put
one point alone beyond what a check admits: the small mass needle (1 + 3e-11 on one entry) and, for Jac0inv, which no
pointer can write, the far corner vertex of the last zone moved by 1.45e-12 h (Q2Q1) / 1.1e-12 h (Q3Q2): the gradient of
its basis function peaks at the zone's last quadrature point, 1.28e-12 / 1.30e-12 there against <= 0.79e-12 elsewhere.

Measured on an MI355X, worst over the cases (bar): A, stored table: mass products 4.2e-16, K1 E-vector 6.4e-16, (d, A d)
5.9e-16, reassembled diagonal 1.8e-15 (1e-13), energy CG 1.3e-11 (1e-8); restored table: the bits of before, every case.
B: stressJinvT 7.9e-14, dt 7.7e-14 (1e-12), dx/dt exact, dv/dt 7.6e-14, de/dt 2.4e-13 (1e-9).  C: set-up data 4.5e-14
(Jac0inv at Q5Q4; 1e-13), volume against the exact sum 1.3e-15, force operators 4.3e-16, mass operators 5.6e-15, H1 CG
1.3e-14, K1 E-vector 1.4e-14, (d, A d) 2.8e-15 (2e-12), K2 r 7.5e-16 d 1.7e-14 x 4.6e-15 (r, z) 1.5e-15 (1e-13), energy CG
1.5e-11, stressJinvT 4.5e-14, dt 7.8e-14, dv/dt 4.2e-14, de/dt 1.1e-13 (1e-10).  D: set-up data 4.6e-14, mass products
9.4e-15, K1 E-vector 2.6e-14, (d, A d) 8.4e-15 (2e-12), energy CG 2.1e-11, stressJinvT 8.6e-14, dt 8.3e-14, dv/dt 9.1e-14,
de/dt 1.4e-13.  E: F^T v 3.1e-14 (1e-12) on all three paths; every ulp, -0.0 and NaN needle poisoned.  F: -F.x 3.2e-14.
Mutations (scratch builds, not committed) and what failed:
  mass_rank1_k reporting zones < 256 only    test_one_mass_entry, test_small_mass_needle [pos2, pos3], ..._energy_cg, ..._special_values
  mass_rank1_k skipping the last point       test_small_mass_needle [pos1, pos3], test_mass_entry_across_the_threshold
  jac0_compact_k reporting zones < 64 only   test_one_curved_zone [zone2, zone3], test_curved_zone_across_the_threshold
  jac0_compact_k skipping the last point     test_corner_vertex_needle [Q2Q1, Q3Q2]
  `mirror` returning 1                       test_skewed_rule, test_one_table_entry, test_table_entry_off_by_1e_13_is_seen
  the weights check returning "ok"           test_weights_that_are_no_symmetric_tensor_product (71 cases), test_skewed_rule
  vec_differs_k without its tail line        the three velocity tests, [Q2Q1-copy] / [copy]
  not_all_ones_k looking at 256 entries      test_one_entry_of_one
The module - 378 tests, contexts shared per configuration - takes 9 s."""

import numpy as np
import pytest

import needle_cases as nc
import shape_cases as sc
import test_gpu_shapes_operators as so
from helpers import deformed_state, make_gpu, make_oracle, rel_err, seeded
from test_gpu_k2 import _run_k2
from test_gpu_qupdate_edges import device_qupdate, oracle_results

pytestmark = pytest.mark.gpu

TOL = nc.BAR_STORED
SWITCHES = so.SWITCHES + ("LGH_B_SYM", "LGH_MASS_SEP", "LGH_MASS_RANK1_TOL", "LGH_JAC0_TOL", "LGH_Q_TINY_GRAD", "LGH_OVERLAP", "LGH_FUSED_INIT")
oid = sc.order_id


# ---- contexts, shared per configuration ----------------------------------------------------------------------------------
class Box:
    def __init__(self, prob, g, o):
        self.prob, self.g, self.o = prob, g, o

    def close(self):
        self.g.close()
        if self.o is not None:
            self.o.close()


def make_pair(prob, env=None, oracle=True, cg_tol=sc.CG_TOL, cg_cap=sc.CG_CAP):
    """a device operator created under `env` (every switch is read once, when the context is created) and an oracle"""
    mp = pytest.MonkeyPatch()
    try:
        for k in SWITCHES:
            mp.delenv(k, raising=False)
        for k, v in (env or {}).items():
            mp.setenv(k, v)
        g = make_gpu(prob, cg_tol=cg_tol, cg_max_iter=cg_cap)
    finally:
        mp.undo()
    return Box(prob, g, make_oracle(prob, cg_tol=cg_tol, cg_max_iter=cg_cap) if oracle else None)


class Boxes:
    """the most recently used configurations stay open (tests of one configuration follow each other)"""

    def __init__(self, keep=6):
        self.keep, self.items = keep, {}

    def get(self, key, make):
        if key in self.items:
            self.items[key] = self.items.pop(key)
        else:
            while len(self.items) >= self.keep:
                self.items.pop(next(iter(self.items))).close()
            self.items[key] = make()
        return self.items[key]

    def close(self):
        while self.items:
            self.items.popitem()[1].close()


@pytest.fixture(scope="module")
def boxes():
    b = Boxes()
    yield b
    b.close()


def expected_k1(order, variant, compact, h1_sym=True, tensor=True):
    """lgh_vcg_k1.hip::vcg_resolve_k1 below the slab threshold of 20 000 zones"""
    if order == (3, 2) and variant == "4":
        return "slab"
    if ((variant is None and order[0] >= 4) or variant == "5") and tensor and compact:
        return "kron"
    if variant == "0" or (order[0] >= 4 and not h1_sym):
        return "column"
    return "plane"


def expected_l2(dim, order, compact, l2_sym=True, tensor=True):
    """lgh_mass.hip::l2_mass_kernel: (2 Kronecker / 1 plane / 0 column, whether it reads compact data)"""
    if dim == 3 and tensor and compact:
        return 2, 1
    if dim == 3 and l2_sym and order[1] >= 2:
        return 1, int(compact)
    return 0, 0


# ---- the operators the checks switch: mass products and one launch of K1 ---------------------------------------------------
def add_vectors(b):
    prob, ctx = b.prob, b.g.ctx
    b.xv, b.xe, b.r, b.d_old = seeded(prob.N, 21), seeded(prob.L2V, 22), seeded(3 * prob.N, 101), seeded(3 * prob.N, 102)
    b.dev = {k: ctx.to_dev(getattr(b, k)) for k in ("xv", "xe", "r", "d_old")}


def device_products(b):
    """H1 and L2 mass products, K1's E-vector and (d, A d) of a first and of a later iteration, with d = r / diag + beta
    d_old formed from the device's own diagonal (returned, for the oracle to form the same d)"""
    prob, ctx, N = b.prob, b.g.ctx, b.prob.N
    ctx.mass_set_ess(-1)
    yv, ye = ctx.empty(N), ctx.empty(prob.L2V)
    ctx.mass_mult(0, b.dev["xv"], yv)
    ctx.mass_mult(1, b.dev["xe"], ye)
    ctx.sync()
    out = dict(yv=yv.cpu().numpy(), ye=ye.cpu().numpy())
    if prob.dim == 3:
        dinv = 1.0 / np.asarray(ctx.mass_diag)
        rz = np.array([float(np.dot(b.r[c * N:(c + 1) * N] ** 2, dinv)) for c in range(3)])
        rz_prev = rz * np.array([1.7, 0.6, 1.1])
        out.update(dinv=dinv, beta=rz / rz_prev)
        for first in (True, False):
            yE, den = ctx.test_vcg_k1(b.dev["r"], None if first else b.dev["d_old"], rz, rz_prev, first)
            out[first] = (yE.cpu().numpy().copy(), np.array(den, copy=True))
        out["mask"], out["n_merged"] = ctx.test_vcg_merged_faces()
    return out


def oracle_products(b, dev):
    from oracle.driver import _dp
    prob, o, N = b.prob, b.o, b.prob.N
    out = dict(yv=o.mass_mult(0, b.xv), ye=o.mass_mult(1, b.xe))
    if prob.dim == 3:
        hmap = np.asarray(prob.h1map).reshape(prob.NE, prob.ND)
        for first in (True, False):
            yE, den = np.empty((3, prob.NE * prob.ND)), np.zeros(3)
            for c in range(3):
                d = b.r[c * N:(c + 1) * N] * dev["dinv"]
                if not first:
                    d = d + dev["beta"][c] * b.d_old[c * N:(c + 1) * N]
                xE = np.ascontiguousarray(d[hmap].reshape(-1))
                o.L.lgo_mass_apply_E(o.h, 0, _dp(xE), _dp(yE[c]))
                den[c] = float(np.dot(xE, yE[c]))
            if dev["n_merged"]:   # merged E-vector of the slab K1 (tests/test_gpu_k1.py::_run_case): an x-face reported once
                idx = np.nonzero(dev["mask"])[0]
                for c in range(3):
                    yE[c, idx - prob.ND + (prob.D1D - 1)] += yE[c, idx]
                    yE[c, idx] = 0.0
            out[first] = (yE, den)
    return out


def compare_products(b, tol, what, spaces=(0, 1)):
    """the device's products against the oracle's, to `tol`; returns the device's"""
    dev = device_products(b)
    ref = oracle_products(b, dev)
    fig = {}
    if 0 in spaces:
        fig["M_h1"] = rel_err(dev["yv"], ref["yv"])
    if 1 in spaces:
        fig["M_l2"] = rel_err(dev["ye"], ref["ye"])
    if b.prob.dim == 3 and 0 in spaces:
        for first in (True, False):
            fig[f"K1-E-{'first' if first else 'later'}"] = max(rel_err(dev[first][0][c], ref[first][0][c]) for c in range(3))
            fig[f"K1-den-{'first' if first else 'later'}"] = max(abs(dev[first][1][c] - ref[first][1][c]) / abs(ref[first][1][c]) for c in range(3))
    print(f"FIG {what} (bar {tol:.0e}): " + " ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    for k, v in fig.items():
        assert v < tol, (what, k, v)
    return dev


def same_bits(a, b):
    """the products of device_products bit for bit, NaN positions included"""
    keys = [k for k in ("yv", "ye") if k in a] + [k for k in (True, False) if k in a]
    for k in keys:
        pa, pb = (a[k], b[k]) if isinstance(a[k], np.ndarray) else (np.concatenate([x.reshape(-1) for x in a[k]]), np.concatenate([x.reshape(-1) for x in b[k]]))
        if not np.array_equal(pa, pb, equal_nan=True):
            return False
    return True


def l2_cg(b, what, tol=1e-10, cap=2000):
    import torch
    prob, g, o = b.prob, b.g, b.o
    rhs = seeded(prob.L2V, 13)
    x_o, it_o = o.cg(1, rhs, rel_tol=tol, max_iter=cap)
    assert it_o < cap
    x = g.ctx.zeros(prob.L2V)
    torch.cuda.synchronize()
    it = g.ctx.cg_solve(1, g.ctx.to_dev(rhs), x, tol, cap)
    g.ctx.sync()
    print(f"FIG {what} cg-l2 {rel_err(x.cpu().numpy(), x_o):.2e} iterations {it} {it_o}")
    assert abs(it - it_o) <= max(1, it_o // 10), (it, it_o)
    assert rel_err(x.cpu().numpy(), x_o) < 1e-8


def one_mult(b, what, curved=False):
    """stressJinvT, dt and dS/dt of helpers.deformed_state against the oracle"""
    import torch
    prob, g, o = b.prob, b.g, b.o
    H1V = prob.H1V
    S = deformed_state(prob)
    sj_o, dt_o, dS_o = oracle_results(o, S)
    Sd = g.ctx.to_dev(S)
    sj, dt = device_qupdate(g, Sd)
    dS = g.ctx.zeros(S.size)
    torch.cuda.synchronize()
    g.reset_quadrature_data()
    g.ctx.reset_timers()
    g.mult(Sd, dS)
    g.ctx.sync()
    dS = dS.cpu().numpy()
    fig = dict(sj=rel_err(sj, sj_o), dt=abs(dt - dt_o) / dt_o, dx=rel_err(dS[:H1V], dS_o[:H1V]), dv=rel_err(dS[H1V:2 * H1V], dS_o[H1V:2 * H1V]),
               de=rel_err(dS[2 * H1V:], dS_o[2 * H1V:]))
    print(f"FIG {what} mult: " + " ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert 0.0 < dt_o < np.inf
    assert fig["sj"] < nc.BAR_QDATA and fig["dt"] < nc.BAR_QDATA
    assert fig["dx"] < 1e-13
    bar = 1e-9 if curved else 1e-10
    assert fig["dv"] < bar
    assert fig["de"] < (1e-8 if prob.order_v == 5 and not curved else bar)


# ==== A: one entry of the mass table ==========================================================================================
A_ORDERS = [(2, 1), (3, 2)]
A_ENVS = {"default": None, "column": "0", "plane": "2", "slab": "4", "kron": "5"}   # LGH_VCG_VARIANT
ROUTES = ("setter", "in-place")


def mass_box(boxes, order, envid, rank1=True):
    def make():
        prob = nc.problem(order)
        env = {} if A_ENVS[envid] is None else {"LGH_VCG_VARIANT": A_ENVS[envid]}
        if not rank1:
            env["LGH_MASS_RANK1"] = "0"
        b = make_pair(prob, env, oracle=rank1)
        add_vectors(b)
        b.D0 = np.array(b.g.ctx.massD, copy=True)
        if rank1:
            b.o_D0 = b.o.massD.copy()
            assert rel_err(b.D0, b.o_D0) < TOL
            assert b.g.ctx.mass_data_form() == "rank1" and b.g.ctx.k1_form() == expected_k1(order, A_ENVS[envid], True)
            assert so._l2_form(b.g) == expected_l2(3, order, True)
            b.base = device_products(b)
        return b
    return boxes.get(("A", order, envid, rank1), make)


def write_table(b, D, route):
    ctx = b.g.ctx
    if route == "setter":
        ctx.massD = D                     # (calls lgh_mass_D() again after the write)
    else:
        ctx.write_massD_in_place(D)       # a caller that kept the pointer ...
        ctx.mass_data_changed()           # ... and says so
    if b.o is not None:
        b.o.massD[:] = D


def restore_table(b, route):
    """the table as set up, on both sides - in a `finally`, and without assertions of its own: a failure of the test's
    body is the one that gets reported, and the shared context never keeps a needle"""
    write_table(b, b.D0, route)
    if b.o is not None:
        b.o.massD[:] = b.o_D0


def assert_restored(b):
    """the compact form must be found again, with the bits it had before the needle"""
    assert b.g.ctx.mass_data_form() == "rank1"
    assert same_bits(device_products(b), b.base), "the compact path after the table was restored"


MASS_CASES = [(o, e, i, r) for o in A_ORDERS for e in A_ENVS for i in range(5) for r in ROUTES]


@pytest.mark.parametrize("order,envid,pos,route", MASS_CASES, ids=[f"{oid(o)}-{e}-pos{i}-{r}" for o, e, i, r in MASS_CASES])
def test_one_mass_entry(boxes, order, envid, pos, route):
    """one entry x 1.5: the stored table in every kernel, no Kronecker form anywhere; H1 and L2 products and K1 (every
    form) against the oracle on the same table; then the table as it was: compact again, the same bits as before"""
    b = mass_box(boxes, order, envid)
    prob, ctx = b.prob, b.g.ctx
    z, q = nc.zone_points(prob.NE, prob.NQ)[pos]
    Dn = b.D0.copy()
    Dn[z * prob.NQ + q] *= 1.5
    try:
        write_table(b, Dn, route)
        assert ctx.mass_data_form() == "stored"
        assert ctx.k1_form() == expected_k1(order, A_ENVS[envid], False) != "kron"
        form, compact = so._l2_form(b.g)
        assert form != 2 and compact == 0 and (form, compact) == expected_l2(3, order, False)
        compare_products(b, TOL, f"A {oid(order)} {envid} ({z}, {q}) {route}")
        if route == "in-place" and envid == "default":
            # the diagonal lgh_mass_data_changed reassembled is the diagonal of the operator with the needle in it
            diag = np.asarray(ctx.mass_diag)
            nodes = np.asarray(prob.h1map).reshape(prob.NE, prob.ND)[z]
            worst = 0.0
            for n in nodes:
                e = np.zeros(prob.N)
                e[n] = 1.0
                worst = max(worst, abs(b.o.mass_mult(0, e)[n] - diag[n]) / np.abs(diag).max())
            print(f"FIG A diagonal {worst:.2e}")
            assert worst < TOL
    finally:
        restore_table(b, route)
    assert_restored(b)


L2_CASES = [(o, i) for o in A_ORDERS for i in range(5)]


@pytest.mark.parametrize("order,pos", L2_CASES, ids=[f"{oid(o)}-pos{i}" for o, i in L2_CASES])
def test_one_mass_entry_energy_cg(boxes, order, pos):
    """the same check switches the energy CG's fused update off: the solve on the needled table against the oracle's"""
    b = mass_box(boxes, order, "default")
    z, q = nc.zone_points(b.prob.NE, b.prob.NQ)[pos]
    Dn = b.D0.copy()
    Dn[z * b.prob.NQ + q] *= 1.5
    try:
        write_table(b, Dn, "setter")
        assert b.g.ctx.mass_data_form() == "stored"
        l2_cg(b, f"A {oid(order)} ({z}, {q})")
    finally:
        restore_table(b, "setter")
    assert_restored(b)


VALUES = {"zero": lambda d: 0.0, "negative": lambda d: -abs(d), "inf": lambda d: np.inf, "nan": lambda d: np.nan}
VALUE_CASES = [(o, v) for o in A_ORDERS for v in VALUES]


@pytest.mark.parametrize("order,value", VALUE_CASES, ids=[f"{oid(o)}-{v}" for o, v in VALUE_CASES])
def test_one_mass_entry_special_values(boxes, order, value):
    """0, -|D|, +inf, NaN in the last entry of the last zone: never compact, and every product has the bits - NaN positions
    included - of a context that was told not to look (LGH_MASS_RANK1=0) on the same table"""
    b, ref = mass_box(boxes, order, "default"), mass_box(boxes, order, "default", rank1=False)
    assert ref.g.ctx.mass_data_form() == "stored" and np.array_equal(ref.D0, b.D0)
    Dn = b.D0.copy()
    Dn[-1] = VALUES[value](Dn[-1])
    try:
        write_table(b, Dn, "setter")
        write_table(ref, Dn, "setter")
        assert b.g.ctx.mass_data_form() == "stored" and b.g.ctx.k1_form() != "kron" and so._l2_form(b.g)[0] != 2
        got, want = device_products(b), device_products(ref)
        if value in ("inf", "nan"):
            assert not np.all(np.isfinite(want["yv"])) and not np.all(np.isfinite(want["ye"]))
        assert same_bits(got, want)
    finally:
        write_table(ref, ref.D0, "setter")
        restore_table(b, "setter")
    assert_restored(b)


SMALL_CASES = [(o, i, r) for o in A_ORDERS for i in range(5) for r in ROUTES]


@pytest.mark.parametrize("order,pos,route", SMALL_CASES, ids=[f"{oid(o)}-pos{i}-{r}" for o, i, r in SMALL_CASES])
def test_small_mass_needle(boxes, order, pos, route):
    """the report alone: 1 + 3e-11 on one entry is thirty times what the check admits AT THAT POINT and leaves every other
    point of the zone within half of it (tests/test_needle_cases.py) - a factor 1.5 moves the zone's mean so far that
    every point is off, and a check that skipped the last point would still say stored"""
    b = mass_box(boxes, order, "default")
    z, q = nc.zone_points(b.prob.NE, b.prob.NQ)[pos]
    Dn = b.D0.copy()
    Dn[z * b.prob.NQ + q] *= nc.MASS_SMALL
    try:
        write_table(b, Dn, route)
        assert b.g.ctx.mass_data_form() == "stored" and b.g.ctx.k1_form() != "kron" and so._l2_form(b.g)[0] != 2
    finally:
        restore_table(b, route)
    assert_restored(b)


def test_mass_entry_across_the_threshold(boxes):
    """the report alone: 1 + 4e-12 on one entry is not compact, 1 + 1e-13 is (the check admits 1e-12; the entry and the
    margins: tests/test_needle_cases.py::test_mass_threshold_needles_are_clear_of_rounding)"""
    b = mass_box(boxes, (3, 2), "default")
    k = nc.mass_threshold_position(b.o_D0, b.prob.W, b.prob.NE)
    try:
        for route in ROUTES:
            for factor, form in ((nc.MASS_ABOVE, "stored"), (nc.MASS_BELOW, "rank1"), (nc.MASS_ABOVE, "stored")):
                Dn = b.D0.copy()
                Dn[k] *= factor
                write_table(b, Dn, route)
                spread = nc.mass_spread(Dn, b.prob.W, b.prob.NE)[0].max()
                print(f"FIG A threshold {route} factor 1 + {factor - 1:.0e}: spread of the device's table {spread:.3e} -> {b.g.ctx.mass_data_form()}")
                assert b.g.ctx.mass_data_form() == form, (route, factor)
    finally:
        restore_table(b, "in-place")    # (the last route: the diagonal is reassembled from the table as it was)
    assert_restored(b)


# ==== B: one curved zone ======================================================================================================
B_ORDERS = [(2, 1), (3, 2), (4, 3)]
B_CASES = ([(o, i, {}) for o in B_ORDERS for i in range(len(nc.curved_zones(int(np.prod(nc.MESH_3D[o])))))]
           + [((3, 2), i, {"LGH_Q_OCC4": v}) for v in ("0", "1") for i in range(4)])


@pytest.mark.parametrize("order,zi,env", B_CASES, ids=[f"{oid(o)}-zone{i}-{so._env_id(e)}" for o, i, e in B_CASES])
def test_one_curved_zone(order, zi, env):
    """the bubble node of one zone moved by 0.1 h: point values of Jac0inv and the stored mass table for ALL zones;
    stressJinvT, dt and one right-hand side (viscosity on) against the oracle on the same mesh"""
    base = nc.problem(order)
    zone = nc.curved_zones(base.NE)[zi]
    b = make_pair(nc.OneCurvedZone(base, zone, 0.1), env, cg_tol=1e-13, cg_cap=5000)
    try:
        assert so._int_form(b.g, "lgh_qupdate_form") == 1 and base.use_viscosity()
        assert b.g.ctx.jac0inv_form() == "stored" and b.g.ctx.mass_data_form() == "stored"
        assert rel_err(b.g.ctx.Jac0inv, b.o.Jac0inv) < TOL and rel_err(b.g.ctx.massD, b.o.massD) < TOL
        one_mult(b, f"B {oid(order)} zone {zone} {so._env_id(env)}", curved=True)
    finally:
        b.close()


@pytest.mark.parametrize("order", sorted(nc.CORNER_DELTA), ids=oid)
def test_corner_vertex_needle(order):
    """the report alone: the far corner vertex of the last zone moved by needle_cases.CORNER_DELTA puts Jac0inv beyond the
    1e-12 of the check at the zone's LAST point and nowhere else (1.28e-12 / 1.30e-12 there, <= 0.79e-12 at every other
    point: tests/test_needle_cases.py) - a moved bubble node is off at every point, and a check that skipped the last one
    would still say "stored" for it; this one it would call compact"""
    base = nc.problem(order)
    b = make_pair(nc.OneCurvedZone(base, base.NE - 1, nc.CORNER_DELTA[order], vertex=True))
    try:
        dev = nc.jac0_point_spread(b.g.ctx.Jac0inv, base.NE, base.NQ, 9)
        print(f"FIG B corner {oid(order)}: the device's Jac0inv: last point {dev[-1, -1]:.3e}, every other point <= {np.delete(dev.reshape(-1), -1).max():.3e}")
        assert rel_err(b.g.ctx.Jac0inv, b.o.Jac0inv) < TOL
        assert b.g.ctx.jac0inv_form() == "stored"
    finally:
        b.close()


@pytest.mark.parametrize("order", B_ORDERS, ids=oid)
def test_curved_zone_across_the_threshold(order):
    """the report alone: a shift of 1e-10 h is seen, one of 1e-14 h is rounding (the check admits 1e-12; margins:
    tests/test_needle_cases.py::test_curved_threshold_needles_are_clear_of_rounding)"""
    base = nc.problem(order)
    for zone in nc.curved_zones(base.NE):
        for delta, form in ((nc.CURVE_ABOVE, "stored"), (nc.CURVE_BELOW, "compact")):
            b = make_pair(nc.OneCurvedZone(base, zone, delta), oracle=False)
            try:
                assert b.g.ctx.jac0inv_form() == form, (zone, delta)
            finally:
                b.close()


# ==== C, D: tables and weights =================================================================================================
def table_name(kind, dim, order, arg=None):
    return f"{kind}/{dim}D/{order[0]}.{order[1]}" + ("" if arg is None else f"/{arg}")


def parse_name(name):
    parts = name.split("/")
    return parts[0], int(parts[1][0]), tuple(int(c) for c in parts[2].split(".")), (int(parts[3]) if len(parts) > 3 else None)


def table_config(name):
    """name -> (problem, symmetry of B, of Bl, whether the weights are a symmetric tensor product)"""
    kind, dim, order, arg = parse_name(name)
    base = nc.problem(order, dim=dim)
    if kind == "skew":
        return nc.SkewRule(base, 0.1, 0.3), 0, int(order[1] == 0), False    # (the Bernstein basis of order 0 is the constant 1)
    if kind == "skew-w":
        return nc.SkewRule(base, 0.0, 0.3), 1, 1, False
    if kind in ("B", "Bl"):
        n = base.Q1D * (base.D1D if kind == "B" else base.L1D)
        return nc.TableNeedle(base, kind, nc.table_indices(n)[arg], eps=1e-6), int(kind != "B"), int(kind != "Bl"), True
    if kind == "W":
        return nc.TableNeedle(base, "W", nc.table_indices(base.NQ)[arg], scale=1.0 + 1e-6), 1, 1, False
    assert kind == "W-tiny"
    return nc.TableNeedle(base, "W", nc.table_indices(base.NQ)[1], scale=1.0 + 2.0 ** -46), 1, 1, False


def table_box(boxes, name, variant=None):
    def make():
        prob, h1_sym, l2_sym, tensor = table_config(name)
        b = make_pair(prob, {} if variant is None else {"LGH_VCG_VARIANT": variant})
        b.h1_sym, b.l2_sym, b.tensor = h1_sym, l2_sym, tensor
        add_vectors(b)
        return b
    return boxes.get(("T", name, variant), make)


def found_compact(b):
    """(mass data compact, Jac0inv compact) as the checks must find them, from the oracle's arrays: every zone's spread
    far inside what a check admits, or some zone's far outside (tests/test_needle_cases.py holds the margins)"""
    prob = b.prob
    out = []
    for spread in (nc.mass_spread(b.o.massD, np.asarray(prob.W), prob.NE)[0], nc.jac0_spread(b.o.Jac0inv, prob.NE, prob.NQ, prob.dim ** 2)[0]):
        assert spread.max() <= nc.SPREAD_BELOW or spread.max() >= nc.SPREAD_ABOVE
        out.append(bool(spread.max() <= nc.SPREAD_BELOW))
    return tuple(out)


def check_forms(b, variant):
    """what lgh_create and the device checks must have found, and the kernels that follow from it; returns the bar of
    the mass operators (2e-12 with compact data, 1e-13 with the stored table)"""
    prob, ctx = b.prob, b.g.ctx
    order = (prob.order_v, prob.order_e)
    compact, jac_compact = found_compact(b)
    assert ctx.table_symmetry() == (b.h1_sym, b.l2_sym)
    assert ctx.mass_data_form() == ("rank1" if compact else "stored")
    assert ctx.jac0inv_form() == ("compact" if jac_compact else "stored")
    if prob.dim == 3:
        assert ctx.k1_form() == expected_k1(order, variant, compact, b.h1_sym, b.tensor)
        assert b.tensor or ctx.k1_form() != "kron"
    assert so._l2_form(b.g) == expected_l2(prob.dim, order, compact, b.l2_sym, b.tensor)
    assert b.tensor or so._l2_form(b.g)[0] != 2
    return nc.BAR_COMPACT if compact else TOL


def setup_data(b, what):
    """The arrays of lgh_setup_rho0detj0 against the oracle's, and the volume against the oracle's point values SUMMED
    EXACTLY (problem 1, rho0 = 1: rho0DetJ0w is w detJ0).  The oracle's own volume is a running sum over NE * NQ points and
    is itself off by up to 1.1e-13 on the equal Q4Q3 mesh (6.2e-14 at Q3Q2, 5.1e-14 at Q5Q4; measured against math.fsum of
    the same points, which agrees with the closed form to 8e-16) - the device's was never further than 3e-15 from the exact
    sum; h0 goes with the cube root of the volume and is held to the oracle's as it is."""
    import math
    g, o = b.g, b.o
    vol = math.fsum(o.rho0DetJ0w.tolist())
    fig = dict(rho0DetJ0w=rel_err(g.ctx.rho0DetJ0w, o.rho0DetJ0w), Jac0inv=rel_err(g.ctx.Jac0inv, o.Jac0inv), massD=rel_err(g.ctx.massD, o.massD),
               diag=rel_err(g.ctx.mass_diag, o.diagV), volume=abs(g.volume - vol) / vol, h0=abs(g.h0 - o.h0) / o.h0)
    print(f"FIG {what} setup " + " ".join(f"{k} {v:.2e}" for k, v in fig.items()) + f" (the oracle's running sum: {abs(o.volume - vol) / vol:.2e})")
    assert b.prob.problem == 1 and abs(o.volume - vol) <= 1e-12 * vol      # (the bar tests/test_shape_cases.py holds the oracle's volume to)
    for k, v in fig.items():
        assert v < TOL, (k, v)


def k1_variants(order):
    return [None, "0", "5"] + (["4"] if order == (3, 2) else []) + (["1"] if order == (4, 3) else [])


SKEW = [table_name("skew", d, o) for d, o in [(3, (1, 0)), (3, (2, 1)), (3, (3, 2)), (3, (4, 3)), (3, (5, 4)), (2, (2, 1)), (2, (3, 2))]]
SKEW_PARTS = ["forms", "setup", "force_E", "force_t_E", "force_L", "mass_E0", "mass_E1", "mass_L", "cg_h1", "products", "k2", "cg_l2", "mult"]
SKEW_CASES = [(n, p) for n in SKEW for p in SKEW_PARTS if not (n.startswith("skew/2D") and p == "k2")]


@pytest.mark.parametrize("name,part", SKEW_CASES, ids=[f"{n}-{p}" for n, p in SKEW_CASES])
def test_skewed_rule(boxes, name, part):
    """SkewRule(0.1, 0.3): asymmetric tables, asymmetric weights - no half table in registers, no Kronecker form anywhere,
    the mass data still compact; every operator of tests/test_gpu_shapes_operators.py against the oracle on the same tables"""
    b = table_box(boxes, name)
    prob = b.prob
    order = (prob.order_v, prob.order_e)
    pair = (None, prob, b.g, b.o)
    if part == "forms":
        check_forms(b, None)
    elif part == "setup":
        setup_data(b, name)
    elif part == "force_E":
        so.test_force_mult_E(pair)
    elif part == "force_t_E":
        so.test_force_mult_transpose_E(pair)
    elif part == "force_L":
        so.test_force_operators_L(pair)
    elif part in ("mass_E0", "mass_E1"):
        so.test_mass_apply_E(pair, int(part[-1]))
    elif part == "mass_L":
        so.test_mass_mult_L(pair)
    elif part == "cg_h1":
        so.test_cg_h1_with_essential_component(pair)
    elif part == "products":
        variants = k1_variants(order) if prob.dim == 3 else [None]
        for variant in variants:
            bv = table_box(boxes, name, variant)
            compare_products(bv, check_forms(bv, variant), f"C {name} variant {variant}")
    elif part == "k2":
        _run_k2(prob, 2, True, None)
    elif part == "cg_l2":
        l2_cg(b, f"C {name}")
    else:
        one_mult(b, f"C {name}")


NEEDLE_TABLES = [table_name(w, 3, o, i) for o in A_ORDERS for w in ("B", "Bl") for i in range(3)]


@pytest.mark.parametrize("name", NEEDLE_TABLES)
def test_one_table_entry(boxes, name):
    """1e-6 on one entry of B (of Bl): table_symmetry() (0, 1) ((1, 0)); the mass operator of that space and K1 in every
    form - the Kronecker form runs on the tiles of the table as given - against the oracle on the same table"""
    which, _, order, _ = parse_name(name)
    for variant in (k1_variants(order) if which == "B" else [None]):
        b = table_box(boxes, name, variant)
        tol = check_forms(b, variant)
        # (one entry of B off breaks the partition of unity at that point: the Jacobian, and with it the mass data, varies
        #  inside every zone by some 1e-6 - the stored table and the point values of Jac0inv are what the checks must find;
        #  Bl does not enter the geometry: compact data, and the Kronecker form on the tile of Bl as given)
        assert (b.g.ctx.mass_data_form(), b.g.ctx.jac0inv_form()) == (("stored", "stored") if which == "B" else ("rank1", "compact"))
        assert b.g.ctx.table_symmetry() == ((0, 1) if which == "B" else (1, 0))
        compare_products(b, tol, f"C {name} variant {variant}", spaces=(0,) if which == "B" else (1,))
    if which == "Bl":
        l2_cg(b, f"C {name}")


@pytest.mark.parametrize("order", A_ORDERS, ids=oid)
def test_table_entry_off_by_1e_13_is_seen(order):
    """the report alone: the mirror check admits 1e-14"""
    base = nc.problem(order)
    for i in nc.table_indices(base.Q1D * base.D1D):
        b = make_pair(nc.TableNeedle(base, "B", i, eps=1e-13), oracle=False)
        try:
            assert b.g.ctx.table_symmetry() == (0, 1), i
        finally:
            b.close()


D_ORDERS = [(2, 1), (3, 2), (4, 3), (5, 4)]
WEIGHTS = [table_name(k, 3, o) for o in D_ORDERS for k in ("skew-w", "W-tiny")] + [table_name("W", 3, o, i) for o in D_ORDERS for i in range(3)]
WEIGHT_PARTS = ["forms", "setup", "products", "cg_l2", "mult"]
WEIGHT_CASES = [(n, p) for n in WEIGHTS for p in WEIGHT_PARTS]


@pytest.mark.parametrize("name,part", WEIGHT_CASES, ids=[f"{n}-{p}" for n, p in WEIGHT_CASES])
def test_weights_that_are_no_symmetric_tensor_product(boxes, name, part):
    """one weight x (1 + 1e-6), x (1 + 2^-46), or asymmetric 1-D weights under symmetric tables: no Kronecker form - not even
    when asked for (LGH_VCG_VARIANT=5) - and no weights from scalar registers in the plane kernels; compact mass data"""
    b = table_box(boxes, name)
    order = (b.prob.order_v, b.prob.order_e)
    if part == "forms":
        check_forms(b, None)
        b5 = table_box(boxes, name, "5")
        check_forms(b5, "5")
        assert b5.g.ctx.k1_form() != "kron"
    elif part == "setup":
        setup_data(b, name)
    elif part == "products":
        for variant in k1_variants(order):
            bv = table_box(boxes, name, variant)
            compare_products(bv, check_forms(bv, variant), f"D {name} variant {variant}")
    elif part == "cg_l2":
        l2_cg(b, f"D {name}")
    else:
        one_mult(b, f"D {name}")


# ==== E: F^T v for "the same" velocity ==========================================================================================
def velocity_box(boxes, order):
    def make():
        b = make_pair(nc.problem(order))
        b.S = deformed_state(b.prob)
        b.o.reset_time_step_estimate()
        b.o.qdata_is_current = False
        b.o.update_quadrature_data(b.S)             # the stress both sides keep
        b.Sd = b.g.ctx.to_dev(b.S)
        b.g.reset_quadrature_data()
        b.g.update_quadrature_data(b.Sd)
        assert b.g.ctx.quadrature_generation()[1:] == (1, 1)
        return b
    return boxes.get(("E", order), make)


def placed(b, v, where):
    """the velocity v on the device: "state" - in the state vector itself; "copy" - a buffer of its own (16-byte aligned);
    "shifted" - eight bytes into a buffer of its own"""
    import torch
    ctx, H1V = b.g.ctx, b.prob.H1V
    if where == "state":
        b.Sd[H1V:2 * H1V] = ctx.to_dev(v)
        torch.cuda.synchronize()
        t = b.Sd[H1V:2 * H1V]
    elif where == "copy":
        t = ctx.to_dev(v)
    else:
        t = ctx.to_dev(np.concatenate([[0.0], v]))[1:]
    return t


def expected_path(H1V, where, t):
    aligned = t.data_ptr() % 16 == 0
    assert aligned == (where == "copy" or (where == "state" and H1V % 2 == 0))
    return ("16-byte" + (" + tail" if H1V % 2 else "")) if aligned else "scalar"


V_CASES = [((2, 1), "state"), ((2, 1), "copy"), ((3, 2), "state"), ((3, 2), "shifted")]


@pytest.mark.parametrize("order,where", V_CASES, ids=[f"{oid(o)}-{w}" for o, w in V_CASES])
def test_one_velocity_entry(boxes, order, where):
    """one entry of v off by 50 %: SolveEnergy must multiply with the velocity it is given.  H1V is odd at Q2Q1 (v inside the
    state is not 16-byte aligned: the scalar path; in a buffer of its own: 16-byte loads and the tail) and even at Q3Q2"""
    b = velocity_box(boxes, order)
    prob, ctx, H1V = b.prob, b.g.ctx, b.prob.H1V
    v0 = b.S[H1V:2 * H1V].copy()
    dS, e_rhs = ctx.zeros(b.S.size), ctx.zeros(prob.L2V)
    try:
        t = placed(b, v0, where)
        print(f"FIG E {oid(order)} {where}: {expected_path(H1V, where, t)} path, H1V = {H1V}")
        assert expected_path(H1V, where, t) == {((2, 1), "state"): "scalar", ((2, 1), "copy"): "16-byte + tail", ((3, 2), "state"): "16-byte",
                                                ((3, 2), "shifted"): "scalar"}[(order, where)]
        ref0 = b.o.force_mult_transpose(v0)
        ctx.solve_energy(b.Sd, t, dS, e_rhs, 1e-8, 2)
        ctx.sync()
        fused = e_rhs.cpu().numpy().copy()
        assert rel_err(fused, ref0) < nc.BAR_QDATA
        worst = 0.0
        for k in nc.vector_indices(H1V):
            v = v0.copy()
            v[k] *= 1.5
            t = placed(b, v, where)
            ref = b.o.force_mult_transpose(v)
            ctx.solve_energy(b.Sd, t, dS, e_rhs, 1e-8, 2)
            ctx.sync()
            err = rel_err(e_rhs.cpu().numpy(), ref)
            worst = max(worst, err)
            assert err < nc.BAR_QDATA, (k, err, rel_err(fused, ref))
        print(f"FIG E {oid(order)} {where}: F^T v {worst:.2e}")
        # the velocity of the state again: the product of the update, bit for bit
        t = placed(b, v0, where)
        ctx.solve_energy(b.Sd, t, dS, e_rhs, 1e-8, 2)
        ctx.sync()
        assert np.array_equal(e_rhs.cpu().numpy(), fused)
    finally:
        placed(b, v0, "state")


def poisoned(b, t, dS, e_rhs):
    """SolveEnergy with the stress in registers: True when the right-hand side came back all NaN AND the next dt look raised"""
    from laghos_amd._lib import LghError
    ctx = b.g.ctx
    ctx.solve_energy(b.Sd, t, dS, e_rhs, 1e-8, 2)
    ctx.sync()
    rhs = e_rhs.cpu().numpy()
    try:
        ctx.get_dt_est()
        raised = False
    except LghError as err:
        assert "velocity other than the state" in str(err)
        raised = True
    assert bool(np.isnan(rhs).all()) == raised and (raised or np.all(np.isfinite(rhs)))
    return raised


@pytest.mark.parametrize("order,where", V_CASES, ids=[f"{oid(o)}-{w}" for o, w in V_CASES])
def test_one_velocity_entry_with_the_stress_in_registers(boxes, order, where):
    """lgh_qupdate_store_stress(0) makes "differs" observable: one ulp, -0.0 for +0.0 or a NaN in one entry poisons the
    right-hand side and the next lgh_get_dt_est; the same velocity at another address gives the bits of the fused product"""
    b = velocity_box(boxes, order)
    prob, ctx, H1V = b.prob, b.g.ctx, b.prob.H1V
    S2 = b.S.copy()
    S2[H1V], S2[2 * H1V - 1] = 0.0, 0.0              # +0.0 at both ends of the velocity
    v0 = S2[H1V:2 * H1V].copy()
    dS, e_rhs = ctx.zeros(b.S.size), ctx.zeros(prob.L2V)
    Sd_keep = b.Sd
    try:
        b.Sd = ctx.to_dev(S2)
        ctx.qupdate_store_stress(0)
        b.g.reset_quadrature_data()
        b.g.update_quadrature_data(b.Sd)
        assert so._int_form(b.g, "lgh_qupdate_stores_stress") == 0
        fused = ctx.empty(prob.L2V)
        assert ctx.fused_force_mult_transpose(fused)
        ctx.sync()
        fused = fused.cpu().numpy().copy()
        assert not poisoned(b, placed(b, v0, where), dS, e_rhs)
        assert np.array_equal(e_rhs.cpu().numpy(), fused)
        needles = [(k, np.nextafter(v0[k], np.inf)) for k in nc.vector_indices(H1V)[1:4]]
        needles += [(k, -0.0) for k in (0, H1V - 1)] + [(k, np.nan) for k in (0, H1V - 1)]
        for k, value in needles:
            v = v0.copy()
            v[k] = value
            assert v.tobytes() != v0.tobytes()
            assert poisoned(b, placed(b, v, where), dS, e_rhs), (k, value)
        assert not poisoned(b, placed(b, v0, where), dS, e_rhs)
        assert np.array_equal(e_rhs.cpu().numpy(), fused)
    finally:
        ctx.qupdate_store_stress(1)
        b.Sd = Sd_keep
        b.g.reset_quadrature_data()
        b.g.update_quadrature_data(b.Sd)


@pytest.mark.parametrize("where", ["state", "copy"])
def test_one_velocity_entry_where_the_grid_strides(where):
    """70^3 zones at Q1Q0: H1V = 3 * 71^3 = 1 073 733 > 2 * 2048 * 256, the smallest 3D mesh on which the capped grid of
    vec_differs_k walks its vector more than once (and H1V is odd: the scalar path inside the state, 16-byte loads and the
    tail in a buffer of its own).  No oracle: the stress stays in registers, a differing entry is NaN and an error."""
    from oracle.fem import Problem
    n = 70
    prob = Problem(breaks=[np.linspace(0.0, 1.0, n + 1)] * 3, order_v=1, order_e=0, problem=1)
    H1V = prob.H1V
    assert 3 * n ** 3 <= 2 * 2048 * 256 < H1V and H1V % 2 == 1    # (69^3 zones have 3 * 70^3 = 1 029 000 entries: below)
    b = make_pair(prob, oracle=False)
    try:
        ctx = b.g.ctx
        b.S = deformed_state(prob)
        v0 = b.S[H1V:2 * H1V].copy()
        b.Sd = ctx.to_dev(b.S)
        ctx.qupdate_store_stress(0)
        b.g.reset_quadrature_data()
        b.g.update_quadrature_data(b.Sd)
        assert so._int_form(b.g, "lgh_qupdate_stores_stress") == 0
        dS, e_rhs = ctx.zeros(b.S.size), ctx.zeros(prob.L2V)
        assert not poisoned(b, placed(b, v0, where), dS, e_rhs)
        for k in (2 * 2048 * 256 + 1000, H1V - 2, H1V - 1):
            v = v0.copy()
            v[k] = np.nextafter(v0[k], np.inf)
            assert poisoned(b, placed(b, v, where), dS, e_rhs), k
        assert not poisoned(b, placed(b, v0, where), dS, e_rhs)
    finally:
        b.close()


# ==== F: `one` with one entry off =================================================================================================
@pytest.mark.parametrize("order", A_ORDERS, ids=oid)
def test_one_entry_of_one(boxes, order):
    """x = 1 except one entry 0.5: SolveVelocity must form -F.x; x = 1 at another address may use F.1 of the update"""
    import torch
    b = velocity_box(boxes, order)
    prob, ctx = b.prob, b.g.ctx
    H1V, L2V, N = prob.H1V, prob.L2V, prob.N
    assert ctx.quadrature_generation()[1] == 1       # F.1 of the update is on hand: the check decides
    free = np.ones(H1V, dtype=bool)
    for c in range(3):
        free[c * N + np.asarray(prob.ess[c], dtype=np.int64)] = False
    dS, rhs, work = ctx.zeros(b.S.size), ctx.zeros(H1V), ctx.zeros(N)
    cases = [(None, None), ("copy", None)] + [("x", k) for k in (0, 257 + 13, L2V - 1)]
    worst = 0.0
    for kind, k in cases:
        x = np.ones(L2V)
        if k is not None:
            x[k] = 0.5
        ref = b.o.force_mult(x)
        dS.zero_()
        torch.cuda.synchronize()
        ctx.solve_velocity(b.Sd, dS, None if kind is None else ctx.to_dev(x), rhs, work, 1e-8, 2)
        ctx.sync()
        r = rhs.cpu().numpy()
        assert not np.any(r[~free])
        worst = max(worst, rel_err(-r[free], ref[free]))
        assert rel_err(-r[free], ref[free]) < nc.BAR_QDATA, (kind, k)
    print(f"FIG F {oid(order)}: -F.x {worst:.2e}")
