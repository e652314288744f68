"""One application of every operator on element grids that are not powers of two (tests/shape_cases.py), against the oracle.

Every other kernel-level test runs on 4x2x2 ... 64^3 zones: rows of 4, 8, 32, 64 zones, NE a multiple of 16, one mass
factor s_e and one Jac0inv for all zones.  Here the graded mesh of every shape (every zone its own s_e, hx != hy != hz)
carries the set-up data, the force and mass operators, ONE launch of K1 and of K2 in every form the solve can dispatch
(tests/test_gpu_k1.py::_run_case, tests/test_gpu_k2.py::_run_k2: their assertions, these meshes) and the quadrature
update in every build of its body; the equal mesh the L2 solve.  Every form asserts which kernel ran (k1_form,
mass_data_form, jac0inv_form, lgh_qupdate_form, lgh_l2_mass_form, the deferred flag of K2) and, for the merged E-vector
of the slab K1, that the number of merged entries is the one the shape alone gives (shape_cases.n_merged).

Bars are the project's: operators 1e-13 of the largest entry, 2e-12 where the compact mass data is in use
(tests/test_gpu_k1.py), stressJinvT and dt 1e-12 (test_qupdate), the CGs as test_cg_h1 / test_cg_l2.
tests/test_shape_cases.py checks on the oracle alone what these tests take for granted.

One launch of K2 is compared while the oracle's residual after the iteration is still a residual (_k2_iterations): on one
zone at Q2Q1 the CG is exact after its third iteration and what is left is round-off on both sides - iterations 1 and 2
there, 1, 2 and 3 everywhere else.

Measured on an MI355X, worst over all shapes, orders and forms (bar): set-up data 3.4e-14 (1e-13), sum of M 1 against the
box volume 5.1e-15, force operators 6.3e-16 (1e-13), mass operators 1.7e-14 (2e-12, compact data), K1 E-vector 2.7e-14 /
(d, A d) 8.5e-15 with compact data (2e-12) and 6.0e-15 / 2.1e-15 with the stored table (1e-13), K2 r 6.6e-15, d 1.3e-14,
x 4.5e-15, (r, z) 1.6e-15 (1e-13), stressJinvT 8.8e-14 and dt 8.7e-14 (1e-12), force products of the update 6.5e-14
(1e-12), H1 CG solution 1.2e-10 and L2 CG solution 3e-12 to 6e-12 (1e-8); merged entries equal to the shape formula everywhere.
Mutations (not committed): the slab K1 reading the mass factor of the first zone of its set fails the five slab cases of
6x1x1 and of 7x3x2; the per-zone Jac0inv with its yy and zz entries swapped fails all 64 row-form cases of test_qupdate with viscosity (without
it - problem 0 - the update does not read Jac0inv).
The module - 980 tests, some 1700 contexts - takes 12 s."""
import ctypes

import numpy as np
import pytest

import shape_cases as sc
from helpers import deformed_state, make_gpu, make_oracle, rel_err, seeded
from test_gpu_k1 import _run_case
from test_gpu_k2 import _run_k2

pytestmark = pytest.mark.gpu

TOL = 1e-13
SWITCHES = ("LGH_VCG_VARIANT", "LGH_MASS_RANK1", "LGH_MASS_KRON", "LGH_SLAB_MERGE", "LGH_SLAB_DYN", "LGH_KRON_NEB", "LGH_RZ_LIMBS",
            "LGH_K2_SKIP", "LGH_K2P", "LGH_K2_GRID", "LGH_Q_FORM", "LGH_Q_OCC4", "LGH_Q_PPT", "LGH_JAC0_COMPACT",
            "LGH_FUSED_FTV", "LGH_FUSED_F1", "LGH_L2_PLANE", "LGH_L2_FUSED", "LGH_L2_NEB")


def _env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _env_id(env):
    return ",".join(f"{k[4:]}={v}" for k, v in env.items()) or "default"


def _int_form(g, name):
    f = ctypes.c_int(-9)
    from laghos_amd import _lib
    _lib.check(getattr(g.ctx.lib, name)(g.ctx.h, ctypes.byref(f)))
    return f.value


def _l2_form(g):
    """(kernel of the L2 mass apply: 2 Kronecker, 1 plane, 0 column; whether it reads the compact data)"""
    f, c = ctypes.c_int(-9), ctypes.c_int(-9)
    from laghos_amd import _lib
    _lib.check(g.ctx.lib.lgh_l2_mass_form(g.ctx.h, ctypes.byref(f), ctypes.byref(c)))
    return f.value, c.value


# ---- one context and one oracle per (shape, order) on the graded mesh: set-up data, force and mass operators ----------
@pytest.fixture(scope="module", params=sc.all_cases(), ids=sc.case_id)
def pair(request):
    mp = pytest.MonkeyPatch()
    _env(mp, {})
    shape, order = request.param
    prob = sc.make_problem(shape, "graded", order)
    g, o = make_gpu(prob), make_oracle(prob)
    yield shape, prob, g, o
    g.close()
    o.close()
    mp.undo()


def _mass_tol(g):
    return 2e-12 if g.ctx.mass_data_form() == "rank1" else TOL


def test_setup_data(pair):
    shape, prob, g, o = pair
    print(f"FIG setup {max(rel_err(g.ctx.rho0DetJ0w, o.rho0DetJ0w), rel_err(g.ctx.Jac0inv, o.Jac0inv), rel_err(g.ctx.massD, o.massD), rel_err(g.ctx.mass_diag, o.diagV)):.2e}")
    assert rel_err(g.ctx.rho0DetJ0w, o.rho0DetJ0w) < TOL
    assert rel_err(g.ctx.Jac0inv, o.Jac0inv) < TOL
    assert rel_err(g.ctx.massD, o.massD) < TOL
    assert rel_err(g.ctx.mass_diag, o.diagV) < TOL
    assert abs(g.volume - o.volume) / o.volume < TOL
    assert abs(g.h0 - o.h0) / o.h0 < TOL
    # a graded Cartesian mesh is affine zone by zone: both compact forms must be found
    assert g.ctx.mass_data_form() == "rank1" and g.ctx.jac0inv_form() == "compact"
    assert g.ctx.table_symmetry() == (1, 1)
    # the closed forms of tests/test_shape_cases.py on the device's results (problem 1: rho0 = 1)
    vol = sc.box_volume(shape)
    assert abs(float(np.sum(g.ctx.rho0DetJ0w)) - vol) <= 1e-13 * vol
    g.ctx.mass_set_ess(-1)
    for space, n in ((0, prob.N), (1, prob.L2V)):
        y = g.ctx.empty(n)
        g.ctx.mass_mult(space, g.ctx.to_dev(np.ones(n)), y)
        g.ctx.sync()
        print(f"FIG unit-mass {abs(float(np.sum(y.cpu().numpy())) - vol) / vol:.2e}")
        assert abs(float(np.sum(y.cpu().numpy())) - vol) <= _mass_tol(g) * vol, space
        u, w = seeded(n, 401 + space), seeded(n, 403 + space)
        Mu, Mw = g.ctx.empty(n), g.ctx.empty(n)
        ud, wd = g.ctx.to_dev(u), g.ctx.to_dev(w)   # (kept until the sync: the launches are asynchronous)
        g.ctx.mass_mult(space, ud, Mu)
        g.ctx.mass_mult(space, wd, Mw)
        g.ctx.sync()
        Mu, Mw = Mu.cpu().numpy(), Mw.cpu().numpy()
        assert abs(float(u @ Mw) - float(w @ Mu)) <= 1e-13 * np.linalg.norm(u) * np.linalg.norm(Mw), space


def test_force_mult_E(pair):
    from oracle.driver import _dp
    shape, prob, g, o = pair
    sJ = seeded(prob.NE * prob.NQ * prob.dim ** 2, 1)
    xE = seeded(prob.L2V, 2)
    yE_o = np.empty(prob.NE * prob.ND * prob.dim)
    o.L.lgo_force_mult_E(o.h, _dp(sJ), _dp(xE), _dp(yE_o))
    yE = g.ctx.empty(yE_o.size)
    g.ctx.force_mult_E(g.ctx.to_dev(sJ), g.ctx.to_dev(xE), yE)
    g.ctx.sync()
    print(f"FIG force {rel_err(yE.cpu().numpy(), yE_o):.2e}")
    assert rel_err(yE.cpu().numpy(), yE_o) < TOL


def test_force_mult_transpose_E(pair):
    from oracle.driver import _dp
    shape, prob, g, o = pair
    sJ = seeded(prob.NE * prob.NQ * prob.dim ** 2, 4)
    vE = seeded(prob.NE * prob.ND * prob.dim, 5)
    y_o = np.empty(prob.L2V)
    o.L.lgo_force_mult_t_E(o.h, _dp(sJ), _dp(vE), _dp(y_o))
    y = g.ctx.empty(prob.L2V)
    g.ctx.force_mult_transpose_E(g.ctx.to_dev(sJ), g.ctx.to_dev(vE), y)
    g.ctx.sync()
    print(f"FIG force {rel_err(y.cpu().numpy(), y_o):.2e}")
    assert rel_err(y.cpu().numpy(), y_o) < TOL


def test_force_operators_L(pair):
    """ForcePAOperator::Mult / MultTranspose at the L-vector boundary and the adjoint identity w.(F e) = (F^T w).e"""
    shape, prob, g, o = pair
    sJ = seeded(prob.NE * prob.NQ * prob.dim ** 2, 6)
    o.stressJinvT[:] = sJ
    g.ctx.set_stressJinvT(sJ)
    e, w = seeded(prob.L2V, 7), seeded(prob.H1V, 8)
    Fe_o, Ftw_o = o.force_mult(e), o.force_mult_transpose(w)
    Fe, Ftw = g.ctx.empty(prob.H1V), g.ctx.empty(prob.L2V)
    ed, wd = g.ctx.to_dev(e), g.ctx.to_dev(w)   # (kept until the sync: the launches are asynchronous)
    g.ctx.force_mult(ed, Fe)
    g.ctx.force_mult_transpose(wd, Ftw)
    g.ctx.sync()
    Fe, Ftw = Fe.cpu().numpy(), Ftw.cpu().numpy()
    print(f"FIG force {max(rel_err(Fe, Fe_o), rel_err(Ftw, Ftw_o)):.2e}")
    assert rel_err(Fe, Fe_o) < TOL
    assert rel_err(Ftw, Ftw_o) < TOL
    lhs, rhs = float(w @ Fe), float(Ftw @ e)
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1.0)


@pytest.mark.parametrize("space", [0, 1])
def test_mass_apply_E(pair, space):
    from oracle.driver import _dp
    shape, prob, g, o = pair
    n = prob.NE * (prob.ND if space == 0 else prob.NL)
    x = seeded(n, 9 + space)
    y_o = np.empty(n)
    o.L.lgo_mass_apply_E(o.h, space, _dp(x), _dp(y_o))
    y = g.ctx.empty(n)
    g.ctx.mass_apply_E(space, g.ctx.to_dev(x), y)
    g.ctx.sync()
    err = rel_err(y.cpu().numpy(), y_o)
    print(f"FIG mass {err:.2e}")
    assert err < _mass_tol(g)


def test_mass_mult_L(pair):
    """MassPAOperator::Mult without and with the essential rows of every component: exactly zero there"""
    shape, prob, g, o = pair
    x = seeded(prob.N, 11)
    xd = g.ctx.to_dev(x)
    try:
        for comp in range(-1, prob.dim):
            y_o = o.mass_mult(0, x, comp=comp)
            y = g.ctx.empty(prob.N)
            g.ctx.mass_set_ess(comp)
            g.ctx.mass_mult(0, xd, y)
            g.ctx.sync()
            y = y.cpu().numpy()
            print(f"FIG mass {rel_err(y, y_o):.2e}")
            assert rel_err(y, y_o) < _mass_tol(g), comp
            if comp >= 0:
                assert len(prob.ess[comp]) and np.all(y[prob.ess[comp]] == 0.0), comp
    finally:
        g.ctx.mass_set_ess(-1)


def test_cg_h1_with_essential_component(pair):
    """Jacobi-PCG on the scalar H1 mass with the essential dofs of component 1 (graded mesh), as test_cg_h1"""
    import torch
    shape, prob, g, o = pair
    b = seeded(prob.N, 12)
    comp = 1
    if len(prob.ess[comp]):
        b[prob.ess[comp]] = 0.0
    x_o, it_o = o.cg(0, b, comp=comp, rel_tol=1e-10, max_iter=300)
    x = g.ctx.zeros(prob.N)
    g.ctx.mass_set_ess(comp)
    torch.cuda.synchronize()
    it = g.ctx.cg_solve(0, g.ctx.to_dev(b), x, 1e-10, 300)
    g.ctx.sync()
    g.ctx.mass_set_ess(-1)
    print(f"FIG cg-h1 {rel_err(x.cpu().numpy(), x_o):.2e} iterations {it} {it_o}")
    assert abs(it - it_o) <= 1
    assert rel_err(x.cpu().numpy(), x_o) < 1e-8


# ---- K1, one launch (3D) ----------------------------------------------------------------------------------------------
# (id, LGH_VCG_VARIANT, form to ask _run_case for, further environment, mass data forms to run)
K1_Q3Q2 = [
    ("default", None, "plane", {}, (True, False)),
    ("column", "0", "column", {}, (True, False)),
    ("plane", "2", "plane", {}, (True, False)),
    ("slab", "4", "slab", {}, (True, False)),
    ("kron", "5", "kron", {}, (True, False)),
    ("slab-through-the-points", "4", "slab", {"LGH_MASS_KRON": "0"}, (True,)),   # (no compact data: nothing the switch could change)
    ("slab-element-local", "4", "slab", {"LGH_SLAB_MERGE": "0"}, (True, False)),
    ("slab-static-sets", "4", "slab", {"LGH_SLAB_DYN": "0"}, (True, False)),
    ("slab-queued-sets", "4", "slab", {"LGH_SLAB_DYN": "1"}, (True, False)),
]
K1_OTHER = {
    (1, 0): [("default", None, "plane", {}), ("column", "0", "column", {}), ("kron", "5", "kron", {})],
    (2, 1): [("default", None, "plane", {}), ("column", "0", "column", {}), ("kron", "5", "kron", {})],
    (4, 3): [("default", None, "plane", {}), ("column", "0", "column", {}), ("kron", "5", "kron", {}), ("twolane", "1", "plane", {}),
             ("kron-8-zones", "5", "kron", {"LGH_KRON_NEB": "0"})],
    (5, 4): [("default", None, "plane", {}), ("column", "0", "column", {}), ("kron", "5", "kron", {}),
             ("kron-4-zones", "5", "kron", {"LGH_KRON_NEB": "0"})],
}


@pytest.mark.parametrize("form", K1_Q3Q2, ids=[f[0] for f in K1_Q3Q2])
@pytest.mark.parametrize("shape", list(sc.SHAPES_3D), ids=sc.shape_id)
def test_k1_one_launch_q3q2(shape, form, monkeypatch):
    """Q3Q2 on every 3D shape: every form of K1, compact and stored mass data, first and later iteration.  _run_case
    asserts k1_form() and mass_data_form(); the merged slab must have merged exactly the x-faces of its chain sets -
    none on 4x1x1 (no complete set), 1x5x1 and 1x1x5 (a complete set of y- / z-neighbours) and 3x3x3 (rows of 3)."""
    _, variant, ask, env, data_forms = form
    prob = sc.make_problem(shape, "graded", (3, 2))
    for rank1 in data_forms:
        for first in (True, False):
            _env(monkeypatch, env)
            n_merged = _run_case(prob, monkeypatch, variant, ask, rank1, first)
            if variant == "4" and env.get("LGH_SLAB_MERGE") != "0":
                assert n_merged == sc.n_merged(shape), (rank1, first)
            else:
                assert n_merged == 0
    if shape in ((4, 1, 1), (1, 5, 1), (1, 1, 5), (3, 3, 3)):
        assert sc.n_merged(shape) == 0


K1_OTHER_CASES = [(s, o, f) for o in sc.ORDERS_3D_OTHER for s in sc.SHAPES_3D_ALL_ORDERS for f in K1_OTHER[o]]


@pytest.mark.parametrize("shape,order,form", K1_OTHER_CASES, ids=[f"{sc.shape_id(s)}-{sc.order_id(o)}-{f[0]}" for s, o, f in K1_OTHER_CASES])
def test_k1_one_launch_other_orders(shape, order, form, monkeypatch):
    _, variant, ask, env = form
    prob = sc.make_problem(shape, "graded", order)
    for rank1 in (True, False):
        for first in (True, False):
            _env(monkeypatch, env)
            assert _run_case(prob, monkeypatch, variant, ask, rank1, first) == 0


# ---- K2, one launch (3D) ----------------------------------------------------------------------------------------------
# (id, environment, bounded-grid kernel expected, K1 form to assert)
K2_Q3Q2 = [
    ("default", {}, True, None),
    ("slab-merged-exact-rz", {"LGH_VCG_VARIANT": "4"}, True, "slab"),
    ("slab-element-local-exact-rz", {"LGH_VCG_VARIANT": "4", "LGH_SLAB_MERGE": "0"}, True, "slab"),
    ("slab-ticketed-rz", {"LGH_VCG_VARIANT": "4", "LGH_RZ_LIMBS": "0"}, True, "slab"),
    ("round-1-kernel", {"LGH_K2P": "0"}, False, None),
    ("one-range-per-cu", {"LGH_K2_GRID": "1"}, True, None),
    ("64-ranges-per-cu", {"LGH_K2_GRID": "64"}, True, None),
]


def _k2_iterations(prob):
    """The iterations of (1, 2, 3) whose launch says something.  _run_k2 holds r, d and x to 1e-13 of their largest entry.
    The launch forms r - alpha A d with an error of a few 2^-53 of the residual that goes IN; when the oracle's CG has
    converged in that very iteration the residual that comes OUT is that round-off and nothing else, and 1e-13 of it is a
    bar the oracle misses against itself.  An iteration is run while the oracle's residual after it is still above 1e-2
    of the one before it in every component.  One case falls out: one zone at Q2Q1 has 9 free nodes per component with
    three distinct eigenvalues of the Jacobi-scaled mass - the CG is exact after the third iteration, the oracle's
    residual there is 9e-16 of the one before."""
    from test_gpu_k2 import _oracle_iteration
    N, keep = prob.N, []
    o = make_oracle(prob)
    try:
        for it in (1, 2, 3):
            inp, exp = _oracle_iteration(prob, o, it, True)
            r_in, r_out = np.abs(inp["r"]).reshape(3, N).max(axis=1), np.abs(exp["r"]).reshape(3, N).max(axis=1)
            if np.all(r_out[r_in > 0] >= 1e-2 * r_in[r_in > 0]):
                keep.append(it)
    finally:
        o.close()
    return keep


@pytest.mark.parametrize("form", K2_Q3Q2, ids=[f[0] for f in K2_Q3Q2])
@pytest.mark.parametrize("shape", list(sc.SHAPES_3D), ids=sc.shape_id)
def test_k2_one_launch_q3q2(shape, form, monkeypatch):
    """iterations 1, 2 and 3 (without / with the update of x / without) of the oracle's CG; _run_k2 asserts the K1 form the
    tables were built for and which K2 ran (`deferred`)"""
    _, env, bounded, k1 = form
    prob = sc.make_problem(shape, "graded", (3, 2))
    its = _k2_iterations(prob)
    assert its == [1, 2, 3]
    for it in its:
        _env(monkeypatch, env)
        _run_k2(prob, it, bounded, k1)


K2_OTHER_CASES = [(s, o) for o in sc.ORDERS_3D_OTHER for s in sc.SHAPES_3D_ALL_ORDERS]


@pytest.mark.parametrize("shape,order", K2_OTHER_CASES, ids=[f"{sc.shape_id(s)}-{sc.order_id(o)}" for s, o in K2_OTHER_CASES])
def test_k2_one_launch_other_orders(shape, order, monkeypatch):
    prob = sc.make_problem(shape, "graded", order)
    its = _k2_iterations(prob)
    assert its == ([1, 2] if (shape, order) == ((1, 1, 1), (2, 1)) else [1, 2, 3])
    for it in its:
        _env(monkeypatch, {})
        _run_k2(prob, it, True, None)


# ---- the quadrature update ----------------------------------------------------------------------------------------------
Q_ENVS_Q3Q2 = [{}, {"LGH_Q_FORM": "0"}, {"LGH_Q_OCC4": "0"}, {"LGH_Q_OCC4": "1"}, {"LGH_JAC0_COMPACT": "0"},
               {"LGH_FUSED_FTV": "0", "LGH_FUSED_F1": "0"}]
Q_CASES = ([(s, (3, 2), 1, e) for s in sc.SHAPES_3D for e in Q_ENVS_Q3Q2]
           + [((7, 3, 2), (3, 2), 0, {})]                                          # the instantiation without viscosity
           + [(s, o, 1, {}) for o in sc.ORDERS_3D_OTHER for s in sc.SHAPES_3D_ALL_ORDERS]
           + [(s, (5, 4), 1, {"LGH_Q_PPT": "1"}) for s in sc.SHAPES_3D_ALL_ORDERS]
           + [(s, o, 1, {}) for s, o in sc.cases_2d()])


@pytest.mark.parametrize("shape,order,problem,env", Q_CASES,
                         ids=[f"{sc.shape_id(s)}-{sc.order_id(o)}-p{p}-{_env_id(e)}" for s, o, p, e in Q_CASES])
def test_qupdate(shape, order, problem, env, monkeypatch):
    """stressJinvT and the dt estimate on helpers.deformed_state (1e-12, as test_qupdate), in the form asked for; then the
    force products the update formed on the way against the oracle's and against the stand-alone kernels on the device's
    own stress (as test_fused_force_products) - or, with the products unfused, the report that none is on hand."""
    import torch
    _env(monkeypatch, env)
    prob = sc.make_problem(shape, "graded", order, problem=problem)
    g, o = make_gpu(prob), make_oracle(prob)
    try:
        row = prob.dim == 3 and order[0] <= 4 and env.get("LGH_Q_FORM") != "0"
        assert _int_form(g, "lgh_qupdate_form") == (1 if row else 0)
        assert g.ctx.jac0inv_form() == ("stored" if env.get("LGH_JAC0_COMPACT") == "0" else "compact")
        S = deformed_state(prob)
        H1V = prob.H1V
        o.reset_time_step_estimate()
        o.qdata_is_current = False
        o.update_quadrature_data(S)
        g.reset_time_step_estimate()
        g.reset_quadrature_data()
        Sd = g.ctx.to_dev(S)
        torch.cuda.synchronize()
        g.update_quadrature_data(Sd)
        # the force products first: looking at stressJinvT hands the array to the caller, and the products formed from it
        # are no longer vouched for
        fused = "LGH_FUSED_FTV" not in env
        gen, f1_ok, ftv_ok = g.ctx.quadrature_generation()
        assert ftv_ok == (1 if fused else 0) and f1_ok == (1 if fused and prob.dim == 3 else 0)
        one = np.ones(prob.L2V)
        F1_o, Ftv_o = o.force_mult(one), o.force_mult_transpose(S[H1V:2 * H1V].copy())
        ftv, f1 = g.ctx.empty(prob.L2V), g.ctx.empty(H1V)
        assert g.ctx.fused_force_mult_transpose(ftv) == bool(ftv_ok)
        assert g.ctx.fused_force_mult(f1) == bool(f1_ok)
        f1_k, ftv_k = g.ctx.empty(H1V), g.ctx.empty(prob.L2V)
        one_d, v_d = g.ctx.to_dev(one), Sd[H1V:2 * H1V].contiguous()
        g.ctx.force_mult(one_d, f1_k)
        g.ctx.force_mult_transpose(v_d, ftv_k)
        g.ctx.sync()
        f1_k, ftv_k = f1_k.cpu().numpy(), ftv_k.cpu().numpy()
        print(f"FIG force-products {max(rel_err(f1_k, F1_o), rel_err(ftv_k, Ftv_o)):.2e}")
        assert rel_err(f1_k, F1_o) < 1e-12 and rel_err(ftv_k, Ftv_o) < 1e-12
        if ftv_ok:
            assert rel_err(ftv.cpu().numpy(), Ftv_o) < 1e-12
            assert rel_err(ftv.cpu().numpy(), ftv_k) < TOL
        if f1_ok:
            assert rel_err(f1.cpu().numpy(), F1_o) < 1e-12
            assert rel_err(f1.cpu().numpy(), f1_k) < TOL
        dt_g, dt_o = g.ctx.get_dt_est(), o.L.lgo_get_dt_est(o.h)
        e_sj = rel_err(g.ctx.stressJinvT, o.stressJinvT)
        print(f"FIG qupdate stress {e_sj:.2e} dt {abs(dt_g - dt_o) / dt_o:.2e}")
        assert e_sj < 1e-12
        assert 0.0 < dt_o < np.inf and abs(dt_g - dt_o) / dt_o < 1e-12
    finally:
        g.close()
        o.close()


# ---- the L2 side: the energy CG on the equal mesh ----------------------------------------------------------------------
def _l2_envs(dim, order):
    """(environment, expected lgh_l2_mass_form): the default and every switch that selects another kernel at this order"""
    if dim == 2:
        return [({}, 0)]
    out = [({}, 2), ({"LGH_L2_FUSED": "0"}, 2)]
    plane = order[1] >= 2    # the plane form exists at L1D = 3, 4, 5 (Q3Q2 and above)
    out.append(({"LGH_MASS_KRON": "0"}, 1 if plane else 0))   # (the Kronecker form is the default wherever the data is compact)
    if plane:
        out.append(({"LGH_MASS_KRON": "0", "LGH_L2_PLANE": "0"}, 0))
    if order == (5, 4):
        out.append(({"LGH_L2_NEB": "0"}, 2))
    return out


L2_CASES = [(s, o, e, f) for s, o in sc.all_cases() for e, f in _l2_envs(len(s), o)]


@pytest.mark.parametrize("shape,order,env,form", L2_CASES, ids=[f"{sc.shape_id(s)}-{sc.order_id(o)}-{_env_id(e)}" for s, o, e, f in L2_CASES])
def test_cg_l2_on_the_equal_mesh(shape, order, env, form, monkeypatch):
    import torch
    _env(monkeypatch, env)
    prob = sc.make_problem(shape, "equal", order)
    g, o = make_gpu(prob), make_oracle(prob)
    try:
        assert g.ctx.mass_data_form() == "rank1"
        assert _l2_form(g)[0] == form
        b = seeded(prob.L2V, 13)
        x_o, it_o = o.cg(1, b, rel_tol=1e-10, max_iter=300)
        assert it_o < 300
        x = g.ctx.zeros(prob.L2V)
        torch.cuda.synchronize()
        it = g.ctx.cg_solve(1, g.ctx.to_dev(b), x, 1e-10, 300)
        g.ctx.sync()
        print(f"FIG cg-l2 {rel_err(x.cpu().numpy(), x_o):.2e} iterations {it} {it_o}")
        assert abs(it - it_o) <= max(1, it_o // 10), (it, it_o)
        assert rel_err(x.cpu().numpy(), x_o) < 1e-8
    finally:
        g.close()
        o.close()
