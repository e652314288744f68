"""GPU parity tests, kernel granularity: every HIP kernel is called through the
C ABI (liblaghos_hip.so) and compared with the CPU oracle on the same seeded
inputs.  Tolerances: the oracle follows the reference's summation order
(x, y, z) with -ffp-contract=off; the HIP kernels contract in a different order
and allow FMA contraction, so agreement is at round-off: <= 1e-13
relative to the largest entry (SURVEY §8c "Tolerances to state")."""
import numpy as np
import pytest

from helpers import deformed_state, make_gpu, make_oracle, rel_err, seeded

pytestmark = pytest.mark.gpu

TOL = 1e-13

CONFIGS = [
    # (mesh, rs, order_v, order_e) -> kernel ids 0x234, 0x246, 0x334, 0x346, 0x358, 0x322,
    # 0x222, 0x26A, and 0x36A (Q5Q4: not instantiated in the reference, laghos_assembly.cpp:544-547;
    # oracle-only parity, BASELINE config 5)
    ("square01_quad", 2, 2, 1),
    ("square01_quad", 1, 3, 2),
    ("cube01_hex", 1, 2, 1),
    ("cube01_hex", 1, 3, 2),
    ("cube01_hex", 0, 4, 3),
    ("cube01_hex", 1, 1, 0),
    ("box01_hex", 0, 3, 2),
    ("cube01_hex", 0, 5, 4),
    # 0x222 and 0x26A: both instantiated by the reference (laghos_assembly.cpp:538-542)
    ("square01_quad", 2, 1, 0),
    ("square01_quad", 0, 5, 4),
]


@pytest.fixture(scope="module", params=CONFIGS, ids=lambda c: f"{c[0]}-rs{c[1]}-Q{c[2]}Q{c[3]}")
def pair(request):
    from oracle.fem import Problem
    mesh, rs, ok, ot = request.param
    prob = Problem(mesh=mesh, rs=rs, order_v=ok, order_e=ot, problem=1)
    g, o = make_gpu(prob), make_oracle(prob)
    yield prob, g, o
    g.close()
    o.close()


def test_tables_are_found_symmetric(pair):
    """The plane-form mass kernels (lockstep K1, L2 mass at Q3Q2 and above) hold half of the 1-D table and are only
    dispatched when lgh_create finds it mirror symmetric to round-off - which every order in use must be, or the
    solves silently run the slower column forms."""
    prob, g, o = pair
    assert g.ctx.table_symmetry() == (1, 1)


def test_setup_data(pair):
    """Rho0DetJ0Vol + mass PA data + Jacobi diagonal (laghos_solver.cpp:1170-1261)"""
    prob, g, o = pair
    assert rel_err(g.ctx.rho0DetJ0w, o.rho0DetJ0w) < TOL
    assert rel_err(g.ctx.Jac0inv, o.Jac0inv) < TOL
    assert rel_err(g.ctx.massD, o.massD) < TOL
    assert rel_err(g.ctx.mass_diag, o.diagV) < TOL
    assert abs(g.volume - o.volume) / o.volume < TOL
    assert abs(g.h0 - o.h0) / o.h0 < TOL


def test_force_mult_E(pair):
    import ctypes
    prob, g, o = pair
    nq = prob.NE * prob.NQ * prob.dim ** 2
    sJ = seeded(nq, 1)
    xE = seeded(prob.L2V, 2)
    yE_o = np.empty(prob.NE * prob.ND * prob.dim)
    from oracle.driver import _dp
    o.L.lgo_force_mult_E(o.h, _dp(sJ), _dp(xE), _dp(yE_o))
    yE = g.ctx.empty(yE_o.size)
    g.ctx.force_mult_E(g.ctx.to_dev(sJ), g.ctx.to_dev(xE), yE)
    g.ctx.sync()
    assert rel_err(yE.cpu().numpy(), yE_o) < TOL


def test_force_mult_transpose_E(pair):
    prob, g, o = pair
    from oracle.driver import _dp
    nq = prob.NE * prob.NQ * prob.dim ** 2
    sJ = seeded(nq, 4)
    vE = seeded(prob.NE * prob.ND * prob.dim, 5)
    y_o = np.empty(prob.L2V)
    o.L.lgo_force_mult_t_E(o.h, _dp(sJ), _dp(vE), _dp(y_o))
    y = g.ctx.empty(prob.L2V)
    g.ctx.force_mult_transpose_E(g.ctx.to_dev(sJ), g.ctx.to_dev(vE), y)
    g.ctx.sync()
    assert rel_err(y.cpu().numpy(), y_o) < TOL


def test_force_operators_L(pair):
    """ForcePAOperator::Mult / MultTranspose at the L-vector boundary, incl. the
    restriction transposes, and the adjoint identity w.(F e) = (F^T w).e"""
    prob, g, o = pair
    sJ = seeded(prob.NE * prob.NQ * prob.dim ** 2, 6)
    o.stressJinvT[:] = sJ
    g.ctx.set_stressJinvT(sJ)
    e = seeded(prob.L2V, 7)
    w = seeded(prob.H1V, 8)
    Fe_o = o.force_mult(e)
    Ftw_o = o.force_mult_transpose(w)
    Fe, Ftw = g.ctx.empty(prob.H1V), g.ctx.empty(prob.L2V)
    g.ctx.force_mult(g.ctx.to_dev(e), Fe)
    g.ctx.force_mult_transpose(g.ctx.to_dev(w), Ftw)
    g.ctx.sync()
    Fe, Ftw = Fe.cpu().numpy(), Ftw.cpu().numpy()
    assert rel_err(Fe, Fe_o) < TOL
    assert rel_err(Ftw, Ftw_o) < TOL
    lhs, rhs = float(w @ Fe), float(Ftw @ e)
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1.0)


@pytest.mark.parametrize("space", [0, 1])
def test_mass_apply_E(pair, space):
    prob, g, o = pair
    from oracle.driver import _dp
    n = prob.NE * (prob.ND if space == 0 else prob.NL)
    x = seeded(n, 9 + space)
    y_o = np.empty(n)
    o.L.lgo_mass_apply_E(o.h, space, _dp(x), _dp(y_o))
    y = g.ctx.empty(n)
    g.ctx.mass_apply_E(space, g.ctx.to_dev(x), y)
    g.ctx.sync()
    assert rel_err(y.cpu().numpy(), y_o) < TOL


@pytest.mark.parametrize("comp", [-1, 0, 1])
def test_mass_mult_L(pair, comp):
    """MassPAOperator::Mult with essential rows (laghos_assembly.cpp:117-121)"""
    prob, g, o = pair
    x = seeded(prob.N, 11)
    y_o = o.mass_mult(0, x, comp=comp)
    y = g.ctx.empty(prob.N)
    g.ctx.mass_set_ess(comp)
    g.ctx.mass_mult(0, g.ctx.to_dev(x), y)
    g.ctx.sync()
    y = y.cpu().numpy()
    assert rel_err(y, y_o) < TOL
    if comp >= 0 and len(prob.ess[comp]):
        assert np.all(y[prob.ess[comp]] == 0.0)


def test_qupdate(pair):
    """fused QUpdate vs the oracle's 5-pass version, on a distorted state"""
    prob, g, o = pair
    S = deformed_state(prob)
    o.reset_time_step_estimate()
    o.qdata_is_current = False
    o.update_quadrature_data(S)
    g.reset_time_step_estimate()
    g.reset_quadrature_data()
    Sd = g.ctx.to_dev(S)
    import torch
    torch.cuda.synchronize()
    g.update_quadrature_data(Sd)
    dt_g = g.ctx.get_dt_est()
    dt_o = o.L.lgo_get_dt_est(o.h)
    assert rel_err(g.ctx.stressJinvT, o.stressJinvT) < 1e-12
    assert abs(dt_g - dt_o) / dt_o < 1e-12


def test_cg_h1(pair):
    """Jacobi-PCG on the scalar H1 mass with essential dofs vs the oracle's CG"""
    prob, g, o = pair
    b = seeded(prob.N, 12)
    comp = 1
    if len(prob.ess[comp]):
        b[prob.ess[comp]] = 0.0
    x_o, it_o = o.cg(0, b, comp=comp, rel_tol=1e-10, max_iter=300)
    x = g.ctx.zeros(prob.N)
    g.ctx.mass_set_ess(comp)
    import torch
    torch.cuda.synchronize()
    it = g.ctx.cg_solve(0, g.ctx.to_dev(b), x, 1e-10, 300)
    g.ctx.sync()
    assert abs(it - it_o) <= 1
    assert rel_err(x.cpu().numpy(), x_o) < 1e-8


def test_cg_l2(pair):
    prob, g, o = pair
    b = seeded(prob.L2V, 13)
    x_o, it_o = o.cg(1, b, rel_tol=1e-10, max_iter=300)
    x = g.ctx.zeros(prob.L2V)
    import torch
    torch.cuda.synchronize()
    it = g.ctx.cg_solve(1, g.ctx.to_dev(b), x, 1e-10, 300)
    g.ctx.sync()
    # unpreconditioned CG on the Bernstein mass matrix: at order 4 it needs > 60
    # iterations and the count moves by a few with the summation order and with the rounding of the mass data
    # (compact form, lgh_mass_data_form: 111 against 118 at Q5Q4); the solution is held to 1e-8 either way
    assert abs(it - it_o) <= max(1, it_o // 10), (it, it_o)
    assert rel_err(x.cpu().numpy(), x_o) < 1e-8


def test_hydro_mult(pair):
    """LagrangianHydroOperator::Mult: one RHS evaluation on a distorted state"""
    prob, g, o = pair
    S = deformed_state(prob, seed=21)
    o.cg_tol, g.cg_tol = 1e-14, 1e-14
    dS_o = np.empty_like(S)
    o.qdata_is_current = False
    o.mult(S, dS_o)
    import torch
    Sd = g.ctx.to_dev(S)
    dS = g.ctx.zeros(S.size)
    torch.cuda.synchronize()
    g.reset_quadrature_data()
    g.mult(Sd, dS)
    g.ctx.sync()
    dS = dS.cpu().numpy()
    H1V = prob.H1V
    assert rel_err(dS[:H1V], dS_o[:H1V]) < TOL
    assert rel_err(dS[H1V:2 * H1V], dS_o[H1V:2 * H1V]) < 1e-10
    assert rel_err(dS[2 * H1V:], dS_o[2 * H1V:]) < 1e-10


def test_energies(pair):
    prob, g, o = pair
    S = deformed_state(prob, seed=22)
    ie_o, ke_o = o.internal_energy(S), o.kinetic_energy(S)
    Sd = g.ctx.to_dev(S)
    import torch
    torch.cuda.synchronize()
    ie = g.ctx.internal_energy(Sd[2 * prob.H1V:])
    ke = g.ctx.kinetic_energy(Sd[prob.H1V:2 * prob.H1V])
    assert abs(ie - ie_o) / abs(ie_o) < 1e-12
    assert abs(ke - ke_o) / abs(ke_o) < 1e-12


def test_smallmat_device():
    """device min-eigenpair / min-singular-value vs numpy"""
    import torch
    from oracle.fem import Problem
    prob = Problem(mesh="cube01_hex", rs=0, order_v=2, order_e=1, problem=1)
    g = make_gpu(prob)
    rng = np.random.default_rng(0)
    n = 20000
    A = rng.standard_normal((n, 3, 3))
    A = 0.5 * (A + np.transpose(A, (0, 2, 1)))
    A[::5, 1, 1] = A[::5, 0, 0]
    A[3::11] = 0.0
    for i in range(0, n, 7):
        A[i] = np.diag(rng.standard_normal(3))
    Ad = g.ctx.to_dev(np.transpose(A, (0, 2, 1)).reshape(-1))
    lam, vec = g.ctx.empty(n), g.ctx.empty(3 * n)
    torch.cuda.synchronize()
    g.ctx.test_eig(3, Ad, lam, vec)
    g.ctx.sync()
    lam, vec = lam.cpu().numpy(), vec.cpu().numpy().reshape(n, 3)
    w = np.linalg.eigvalsh(A)
    scale = np.maximum(np.abs(w).max(axis=1), 1e-300)
    scale[scale < 1e-200] = 1.0
    assert np.max(np.abs(lam - w[:, 0]) / scale) < 1e-14
    res = np.linalg.norm(np.einsum("nij,nj->ni", A, vec) - lam[:, None] * vec, axis=1) / scale
    assert np.max(res) < 1e-14
    assert np.max(np.abs(np.linalg.norm(vec, axis=1) - 1.0)) < 1e-14
    J = rng.standard_normal((n, 3, 3))
    sv = g.ctx.empty(n)
    g.ctx.test_singular(3, g.ctx.to_dev(np.transpose(J, (0, 2, 1)).reshape(-1)), sv)
    g.ctx.sync()
    s = np.linalg.svd(J, compute_uv=False)
    # the family rule of test_gpu_smallmat_edges.py: max(1e-14, 4 e_oracle) s_max, e_oracle the oracle's worst error over
    # s_max on these same matrices (both routines form J^T J: the error grows with the condition number, and the worst
    # conditioned of 20 000 Gaussian matrices sets it)
    from smallmat_cases import oracle_sv
    e_oracle = np.max(np.abs(oracle_sv(3, J) - s[:, 2]) / s[:, 0])
    e_device = np.max(np.abs(sv.cpu().numpy() - s[:, 2]) / s[:, 0])
    print(f"singular value: device {e_device:.2e} oracle {e_oracle:.2e}")
    assert e_device <= max(1e-14, 4 * e_oracle)
    assert max(1e-14, 4 * e_oracle) < 1e-10  # (never weaker than the bar this assertion replaced)
    g.close()


def test_device_sqrt():
    """The square root of the small-matrix routines (v_rsq_f64 + one Goldschmidt step + one residual correction, 8
    instructions instead of the 22 of the correctly rounded expansion): within 1 ulp of numpy's over 600 decades,
    exact at 0 and at exact squares; +inf and the signed zeros as the library root returns them."""
    from oracle.fem import Problem
    prob = Problem(mesh="cube01_hex", rs=0, order_v=1, order_e=0, problem=1)
    g = make_gpu(prob)
    try:
        rng = np.random.default_rng(7)
        x = np.concatenate([10.0 ** rng.uniform(-300, 300, 200000), rng.uniform(0.25, 4.0, 200000),
                            np.array([0.0, 1.0, 4.0, 9.0, 2.25, 1e-300, 1e300, 2.0 ** -1000, 2.0 ** 1000])])
        xd = g.ctx.to_dev(x)
        yd = g.ctx.zeros(x.size)
        g.ctx.test_sqrt(xd, yd)
        g.ctx.sync()
        y = yd.cpu().numpy()
        ref = np.sqrt(x)
        assert np.all(np.abs(y - ref) <= np.spacing(ref))
        assert np.array_equal(y[-9:-4], ref[-9:-4])  # 0 and exact squares
        # special values come back as the library root returns them
        sp = np.array([np.inf, -0.0, 0.0])
        sd = g.ctx.to_dev(sp)
        od = g.ctx.zeros(3)
        g.ctx.test_sqrt(sd, od)
        g.ctx.sync()
        out = od.cpu().numpy()
        assert out[0] == np.inf and out[1] == 0.0 and np.signbit(out[1]) and out[2] == 0.0 and not np.signbit(out[2])
    finally:
        g.close()


def test_tg_source_2d():
    """2D Taylor-Green energy source (laghos_solver.cpp:448-467) on a distorted mesh vs the oracle"""
    from oracle.fem import Problem
    from oracle.driver import _dp
    prob = Problem(mesh="square01_quad", rs=2, order_v=2, order_e=1, problem=0)
    g, o = make_gpu(prob), make_oracle(prob)
    S = deformed_state(prob, seed=5)
    want = np.empty(prob.L2V)
    o.L.lgo_qupdate(o.h, _dp(S))
    o.L.lgo_tg_source_2d(o.h, _dp(S), _dp(want))
    got = g.ctx.empty(prob.L2V)
    g.ctx.tg_source_2d(g.ctx.to_dev(S), got)
    g.ctx.sync()
    assert rel_err(got.cpu().numpy(), want) < TOL
    g.close()
    o.close()


def test_problem7_vorticity_and_gravity():
    """Problem 7 (Rayleigh-Taylor): the vorticity-scaled viscosity of QUpdateBody
    (laghos_solver.cpp:1097-1103) and the acceleration source of SolveVelocity (:371-380),
    one QUpdate and one RHS evaluation on a distorted state vs the oracle."""
    import torch
    from oracle.fem import Problem
    prob = Problem(mesh="rt2D", rs=1, order_v=3, order_e=2, problem=7)
    g, o = make_gpu(prob), make_oracle(prob)
    S = deformed_state(prob, seed=3)
    o.reset_time_step_estimate()
    o.qdata_is_current = False
    o.update_quadrature_data(S)
    g.reset_time_step_estimate()
    g.reset_quadrature_data()
    Sd = g.ctx.to_dev(S)
    torch.cuda.synchronize()
    g.update_quadrature_data(Sd)
    assert rel_err(g.ctx.stressJinvT, o.stressJinvT) < 1e-12
    assert abs(g.ctx.get_dt_est() - o.L.lgo_get_dt_est(o.h)) / o.L.lgo_get_dt_est(o.h) < 1e-12
    o.cg_tol, g.cg_tol = 1e-14, 1e-14
    dS_o = np.empty_like(S)
    o.qdata_is_current = False
    o.mult(S, dS_o)
    dS = g.ctx.zeros(S.size)
    g.reset_quadrature_data()
    g.mult(Sd, dS)
    g.ctx.sync()
    assert rel_err(dS.cpu().numpy(), dS_o) < 1e-9
    g.close()
    o.close()


def test_qupdate_shortcut_on_live_sedov_state():
    """The wave-uniform shortcut of the eigen-decomposition (lgh_qupdate_set_tiny_grad; zones the blast has not
    reached) on the state it is meant for: 12 real time steps of 3D Sedov Q3Q2 (512 zones), then the QUpdate of
    that state with the shortcut at its default threshold, restricted to exact zeros, and switched off, and
    the oracle's.  The three device results must agree to <= 1e-14 of the largest entry (the bar the kernel has
    against the oracle is 1e-12), the time-step estimates to 1e-14, and the shortcut must have something to do:
    a part of this state lies below the threshold."""
    import torch
    from laghos_amd.hydro import TimeLoop
    from oracle.fem import Problem
    prob = Problem(mesh="cube01_hex", rs=2, order_v=3, order_e=2, problem=1)
    g, o = make_gpu(prob), make_oracle(prob)
    try:
        loop = TimeLoop(g, t_final=1e9, max_steps=12)
        while loop.step():
            pass
        S = loop.S
        out = {}
        for name, thr in (("default", 1e-30), ("zeros", 0.0), ("off", -1.0)):
            g.ctx.qupdate_set_tiny_grad(thr)
            g.reset_time_step_estimate()
            g.reset_quadrature_data()
            g.update_quadrature_data(S)
            out[name] = (g.ctx.stressJinvT.copy(), g.ctx.get_dt_est())
        g.ctx.qupdate_set_tiny_grad(1e-30)
        ref, dt_ref = out["off"]
        for name in ("default", "zeros"):
            sj, dt = out[name]
            assert rel_err(sj, ref) <= 1e-14, name
            assert abs(dt - dt_ref) <= 1e-14 * dt_ref, name
        Sh = S.cpu().numpy()
        o.reset_time_step_estimate()
        o.qdata_is_current = False
        o.update_quadrature_data(Sh)
        assert rel_err(out["default"][0], o.stressJinvT) < 1e-12
        assert abs(out["default"][1] - o.L.lgo_get_dt_est(o.h)) / dt_ref < 1e-12
        # the state does contain such points (exact zeros and tails of the CG iterations)
        v = Sh[prob.H1V:2 * prob.H1V]
        assert np.mean(np.abs(v) <= 1e-30) > 0.02
    finally:
        g.close()
        o.close()


@pytest.mark.parametrize("order", [(4, 3), (5, 4)], ids=["Q4Q3", "Q5Q4"])
def test_lockstep_k1_forms_agree_at_high_order(order, monkeypatch):
    """The lockstep velocity solve at D1D >= 5 through each form of its mass-apply kernel (LGH_VCG_VARIANT:
    0 = column form, 1 = plane form with two lanes per plane, default = plane form as dispatched): 16 zones
    (a ragged last batch for the batches of 5), distorted state, CG to 1e-14: the velocity part of dS/dt
    agrees with the oracle to the operator tolerance in every form."""
    from oracle.fem import Problem
    prob = Problem(mesh="box01_hex", rs=0, order_v=order[0], order_e=order[1], problem=1)
    S = deformed_state(prob, seed=33)
    o = make_oracle(prob)
    try:
        o.cg_tol = 1e-14
        dS_o = np.empty_like(S)
        o.qdata_is_current = False
        o.mult(S, dS_o)
    finally:
        o.close()
    H1V = prob.H1V
    for variant in ("0", "1", None):
        if variant is None:
            monkeypatch.delenv("LGH_VCG_VARIANT", raising=False)
        else:
            monkeypatch.setenv("LGH_VCG_VARIANT", variant)
        g = make_gpu(prob)
        try:
            g.cg_tol = 1e-14
            Sd = g.ctx.to_dev(S)
            dS = g.ctx.zeros(S.size)
            g.reset_quadrature_data()
            g.mult(Sd, dS)
            g.ctx.sync()
            dS = dS.cpu().numpy()
        finally:
            g.close()
        assert rel_err(dS[H1V:2 * H1V], dS_o[H1V:2 * H1V]) < 1e-10, variant


@pytest.mark.parametrize("mesh,rs", [("box01_hex", 0), ("cube01_hex", 1)], ids=["16zones", "64zones"])
def test_lockstep_k1_forms_agree_at_q3q2(mesh, rs, monkeypatch):
    """The lockstep velocity solve at Q3Q2 (kernel id 0x346, the headline configuration) through each form of its
    mass-apply kernel (LGH_VCG_VARIANT: 0 = column form, 2 = plane form, 4 = slab form, lgh_vcg_slab.hip; default = as
    dispatched; the matrix-core form of round 3 has left the library: profiles/experiments/r3_lgh_vcg_mfma.hip).  16 and 64
    zones: ragged last sets for the sets of 5 elements of the slab form and the batches of 13 of the plane form.  Distorted state, CG to 1e-14: the velocity part of
    dS/dt agrees with the oracle to the operator tolerance in every form."""
    from oracle.fem import Problem
    prob = Problem(mesh=mesh, rs=rs, order_v=3, order_e=2, problem=1)
    S = deformed_state(prob, seed=37)
    o = make_oracle(prob)
    try:
        o.cg_tol = 1e-14
        dS_o = np.empty_like(S)
        o.qdata_is_current = False
        o.mult(S, dS_o)
    finally:
        o.close()
    H1V = prob.H1V
    for variant in ("0", "2", "4", None):
        if variant is None:
            monkeypatch.delenv("LGH_VCG_VARIANT", raising=False)
        else:
            monkeypatch.setenv("LGH_VCG_VARIANT", variant)
        g = make_gpu(prob)
        try:
            if variant == "4":
                assert g.ctx.k1_form() == "slab"
            g.cg_tol = 1e-14
            Sd = g.ctx.to_dev(S)
            dS = g.ctx.zeros(S.size)
            g.reset_quadrature_data()
            g.mult(Sd, dS)
            g.ctx.sync()
            dS = dS.cpu().numpy()
        finally:
            g.close()
        assert rel_err(dS[H1V:2 * H1V], dS_o[H1V:2 * H1V]) < 1e-10, variant


def _fused_state(kind, prob, g):
    """deformed: a seeded distorted state; sedov: the live state after 12 real time steps"""
    if kind == "deformed":
        return g.ctx.to_dev(deformed_state(prob, seed=41))
    from laghos_amd.hydro import TimeLoop
    loop = TimeLoop(g, t_final=1e9, max_steps=12)
    while loop.step():
        pass
    return loop.S


@pytest.mark.parametrize("kind", ["deformed", "sedov"])
@pytest.mark.parametrize("cfg", [("cube01_hex", 1, 3, 2), ("cube01_hex", 1, 2, 1), ("cube01_hex", 0, 4, 3), ("square01_quad", 1, 3, 2)],
                         ids=lambda c: f"{c[0]}-rs{c[1]}-Q{c[2]}Q{c[3]}")
def test_fused_force_products(cfg, kind):
    """The force products the production step uses are formed inside the fused QUpdate kernel
    (lgh_qupdate -> force_e_q / erhs_q), not by force_mult_3d / force_mult_t_3d.  Here they are taken out through
    lgh_fused_force_mult / _transpose and compared, at the force kernels' own tolerance, with
      * the oracle's ForceMult(one) and ForceMultTranspose(v) (laghos_assembly.cpp:296-514, :715-924) on the
        oracle's quadrature data of the same state, and
      * the stand-alone HIP kernels on the device's own quadrature data (lgh_set_fused_forces(ctx, 0) path),
    on a distorted random state and on a live Sedov state.  2D forms only F^T v inside the update."""
    from oracle.fem import Problem
    mesh, rs, ok, ot = cfg
    prob = Problem(mesh=mesh, rs=rs, order_v=ok, order_e=ot, problem=1)
    g, o = make_gpu(prob), make_oracle(prob)
    try:
        S = _fused_state(kind, prob, g)
        Sh = S.cpu().numpy()
        H1V = prob.H1V
        g.reset_quadrature_data()
        g.update_quadrature_data(S)
        gen, f1_ok, ftv_ok = g.ctx.quadrature_generation()
        assert ftv_ok == 1 and f1_ok == (1 if prob.dim == 3 else 0)
        o.qdata_is_current = False
        o.update_quadrature_data(Sh)
        one = np.ones(prob.L2V)
        F1_o = o.force_mult(one)
        Ftv_o = o.force_mult_transpose(Sh[H1V:2 * H1V].copy())
        # fused products
        ftv = g.ctx.empty(prob.L2V)
        assert g.ctx.fused_force_mult_transpose(ftv)
        g.ctx.sync()
        ftv = ftv.cpu().numpy()
        assert rel_err(ftv, Ftv_o) < 1e-12   # (the fused update's own bar against the oracle's quadrature data)
        f1 = None
        if prob.dim == 3:
            f1 = g.ctx.empty(H1V)
            assert g.ctx.fused_force_mult(f1)
            g.ctx.sync()
            f1 = f1.cpu().numpy()
            assert rel_err(f1, F1_o) < 1e-12
        # the stand-alone kernels on the device's own stressJinvT: same operator, same data -> the kernel tolerance
        f1_k, ftv_k = g.ctx.empty(H1V), g.ctx.empty(prob.L2V)
        g.ctx.force_mult(g.ctx.to_dev(one), f1_k)
        g.ctx.force_mult_transpose(S[H1V:2 * H1V].contiguous(), ftv_k)
        g.ctx.sync()
        assert rel_err(ftv, ftv_k.cpu().numpy()) < TOL
        if f1 is not None:
            assert rel_err(f1, f1_k.cpu().numpy()) < TOL
        # (force_mult hands out nothing mutable: the products are still on hand) ... until the data is reset
        assert g.ctx.quadrature_generation()[1:] == (f1_ok, 1)
        g.ctx.reset_quadrature_data()
        assert g.ctx.quadrature_generation()[1:] == (0, 0)
        assert not g.ctx.fused_force_mult_transpose(g.ctx.empty(prob.L2V))
    finally:
        g.close()
        o.close()


def test_stress_kept_in_registers():
    """lgh_qupdate_store_stress(ctx, 0): the update forms F.1 and F^T v from the stress in registers and does not write
    the nine stressJinvT planes.  One right-hand-side evaluation must give the SAME BITS as with the planes written (the
    products are formed from the same registers either way), the array in memory must stay untouched, every reader of
    it must refuse loudly, and a SolveEnergy for a velocity other than the state's (what RK2Avg does) must end in NaN
    plus an error at the next lgh_get_dt_est - never in numbers computed from stale stress."""
    from laghos_amd._lib import LghError
    from oracle.fem import Problem
    prob = Problem(mesh="cube01_hex", rs=1, order_v=3, order_e=2, problem=1)
    S = deformed_state(prob, seed=71)
    g = make_gpu(prob)
    try:
        ctx = g.ctx
        Sd = ctx.to_dev(S)
        dS1, dS2 = ctx.zeros(S.size), ctx.zeros(S.size)
        g.reset_quadrature_data()
        g.mult(Sd, dS1)
        ctx.sync()
        stress_written = np.array(ctx.stressJinvT, copy=True)
        assert np.abs(stress_written).max() > 0
        marker = np.full_like(stress_written, 7.25)
        ctx.set_stressJinvT(marker)
        ctx.qupdate_store_stress(0)
        g.reset_quadrature_data()
        g.mult(Sd, dS2)
        ctx.sync()
        assert np.array_equal(dS1.cpu().numpy(), dS2.cpu().numpy())
        # (reading the array through the property hands it to the caller - do that last)
        one = ctx.to_dev(np.ones(prob.L2V))
        y = ctx.empty(prob.H1V)
        with pytest.raises(LghError, match="kept in registers"):
            ctx.force_mult(one, y)
        with pytest.raises(LghError, match="kept in registers"):
            ctx.force_mult_transpose(Sd[prob.H1V:2 * prob.H1V], ctx.empty(prob.L2V))
        # a velocity that is not the state's: NaN right-hand side, error at the next dt read
        v_other = ctx.to_dev(S[prob.H1V:2 * prob.H1V] * 1.5)
        e_rhs, dS3 = ctx.empty(prob.L2V), ctx.zeros(S.size)
        ctx.solve_energy(Sd, v_other, dS3, e_rhs, 1e-8, 50)
        ctx.sync()
        assert np.isnan(e_rhs.cpu().numpy()).all()
        with pytest.raises(LghError, match="velocity other than the state"):
            ctx.get_dt_est()
        assert np.array_equal(np.asarray(ctx.stressJinvT), marker), "the planes must not have been written"
        # looking at the array does not make planes nobody wrote current: the readers still refuse
        with pytest.raises(LghError, match="kept in registers"):
            ctx.force_mult(one, y)
        # back on: the next update writes them again
        ctx.qupdate_store_stress(1)
        g.reset_quadrature_data()
        g.mult(Sd, dS2)
        ctx.sync()
        assert np.array_equal(np.asarray(ctx.stressJinvT), stress_written)
    finally:
        g.close()


def test_fused_products_follow_content_not_addresses():
    """lgh_solve_energy must use the velocity it is GIVEN (ForcePA->MultTranspose(v, e_rhs),
    laghos_solver.cpp:473), whatever lgh_qupdate saw before:
      * S.v changed in place after lgh_qupdate(S) (no ResetQuadratureData): the reference multiplies the stale
        stress with the NEW v - so must the library (an address-keyed cache returned F^T v_old);
      * the same velocity at another address may use the fused product - and gives the same numbers;
      * a `one` that is not all ones is not treated as one; NULL stands for the operator's own."""
    import torch
    from oracle.fem import Problem
    prob = Problem(mesh="cube01_hex", rs=1, order_v=3, order_e=2, problem=1)
    g, o = make_gpu(prob), make_oracle(prob)
    try:
        H1V, L2V = prob.H1V, prob.L2V
        Sh = deformed_state(prob, seed=43)
        S = g.ctx.to_dev(Sh)
        o.qdata_is_current = False
        o.update_quadrature_data(Sh)            # the stress both sides keep from now on
        g.reset_quadrature_data()
        g.update_quadrature_data(S)
        v_old = Sh[H1V:2 * H1V].copy()
        rng = np.random.default_rng(5)
        v_new = 1.5 * v_old + 0.1 * rng.uniform(-1, 1, H1V)
        ref_old, ref_new = o.force_mult_transpose(v_old), o.force_mult_transpose(v_new)
        assert rel_err(ref_old, ref_new) > 0.1  # the two right-hand sides are far apart
        dS, e_rhs = g.ctx.zeros(Sh.size), g.ctx.zeros(L2V)
        # same content at another address
        v_copy = S[H1V:2 * H1V].clone()
        g.ctx.solve_energy(S, v_copy, dS, e_rhs, 1e-14, 200)
        g.ctx.sync()
        rhs_copy = e_rhs.cpu().numpy().copy()
        assert rel_err(rhs_copy, ref_old) < 1e-12
        # in-place change of the state's velocity, no reset
        S[H1V:2 * H1V] = g.ctx.to_dev(v_new)
        torch.cuda.synchronize()
        g.ctx.solve_energy(S, S[H1V:2 * H1V], dS, e_rhs, 1e-14, 200)
        g.ctx.sync()
        assert rel_err(e_rhs.cpu().numpy(), ref_new) < 1e-12
        # back to the old velocity: the fused product is usable again, and equals what it was
        S[H1V:2 * H1V] = g.ctx.to_dev(v_old)
        torch.cuda.synchronize()
        g.ctx.solve_energy(S, S[H1V:2 * H1V], dS, e_rhs, 1e-14, 200)
        g.ctx.sync()
        assert np.array_equal(e_rhs.cpu().numpy(), rhs_copy)
        # `one`: NULL is the operator's own; a vector that is not all ones goes through ForceMult
        F1_o = o.force_mult(np.ones(L2V))
        x = np.ones(L2V)
        x[::7] = 0.5
        Fx_o = o.force_mult(x)
        rhs, work = g.ctx.zeros(H1V), g.ctx.zeros(prob.N)
        for one_arg, ref in ((None, F1_o), (g.ctx.to_dev(np.ones(L2V)), F1_o), (g.ctx.to_dev(x), Fx_o)):
            dS.zero_()
            torch.cuda.synchronize()
            g.ctx.solve_velocity(S, dS, one_arg, rhs, work, 1e-14, 300)
            g.ctx.sync()
            # rhs_h1 holds -F x with the essential rows zeroed; compare away from them
            r = rhs.cpu().numpy()
            free = r != 0.0
            assert rel_err(-r[free], ref[free]) < 1e-12
    finally:
        g.close()
        o.close()


SLAB_SWITCHES = [
    {},
    {"LGH_SLAB_DYN": "0"},
    {"LGH_SLAB_EXACT": "0"},
    {"LGH_SLAB_WIDE": "0"},
    {"LGH_SLAB_WIDE": "0", "LGH_SLAB_DYN": "0"},
    {"LGH_SLAB_DEFER": "0"},
    {"LGH_RZ_LIMBS": "0"},
    {"LGH_SLAB_YE_WIDE": "1"},
]


@pytest.mark.parametrize("switches", SLAB_SWITCHES, ids=lambda d: ",".join(f"{k.replace('LGH_SLAB_', '').replace('LGH_', '')}={v}" for k, v in d.items()) or "default")
def test_slab_k1_switches(switches, monkeypatch):
    """Every A/B switch of the slab-form K1 (lgh_vcg_slab.hip) selects a different instantiation:
    row loads or node gathers, exact integer accumulation of (d, A d) or the ticketed fold, sets drawn from
    the workgroup's queue or assigned statically.  128 zones (26 sets: a ragged last set),
    distorted state, CG to 1e-14: the velocity part of dS/dt agrees with the oracle to the operator tolerance, and -
    the sums being exact - all schedules with exact accumulation give the same bits.  (r, z) is kept in exact
    accumulators as well unless LGH_RZ_LIMBS=0 or the deferred fold of (d, A d) is off: those two fold (r, z) with the
    ticketed reduction of K2, round it differently, and agree bit for bit with each other."""
    from oracle.fem import Problem
    prob = Problem(mesh="box01_hex", rs=1, order_v=3, order_e=2, problem=1)
    S = deformed_state(prob, seed=39)
    o = make_oracle(prob)
    try:
        o.cg_tol = 1e-14
        dS_o = np.empty_like(S)
        o.qdata_is_current = False
        o.mult(S, dS_o)
    finally:
        o.close()
    H1V = prob.H1V
    monkeypatch.setenv("LGH_VCG_VARIANT", "4")
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    g = make_gpu(prob)
    try:
        assert g.ctx.k1_form() == "slab"
        g.cg_tol = 1e-14
        Sd = g.ctx.to_dev(S)
        dS = g.ctx.zeros(S.size)
        g.reset_quadrature_data()
        g.mult(Sd, dS)
        g.ctx.sync()
        dS = dS.cpu().numpy()
    finally:
        g.close()
    assert rel_err(dS[H1V:2 * H1V], dS_o[H1V:2 * H1V]) < 1e-10
    if "LGH_SLAB_EXACT" not in switches:
        key = "slab_ticket_rz_bits" if ("LGH_SLAB_DEFER" in switches or "LGH_RZ_LIMBS" in switches) else "slab_exact_bits"
        ref = test_slab_k1_switches.__dict__.setdefault(key, dS[H1V:2 * H1V].copy())
        assert np.array_equal(ref, dS[H1V:2 * H1V]), "exact accumulation: the result must not depend on the schedule"


def test_slab_merged_evector_vs_element_local(monkeypatch):
    """Round 5: where the five zones of a slab set are x-neighbours K1 sums the shared x-faces itself and stores 16 rows
    of 16 x-nodes per component (merged E-vector layout, lgh_vcg_tables.hip::slab_merge_layout); LGH_SLAB_MERGE=0 keeps the
    element-local layout of rounds 3 and 4.  512 zones in rows of 8 (chains, sets that straddle two rows, a ragged last
    set), distorted state, CG to 1e-14: both layouts give the oracle's dv/dt to the operator tolerance and agree with
    each other to round-off (the order of the per-node sums differs); within a layout the schedule (workgroup queues or
    static sets) does not move a bit."""
    from oracle.fem import Problem
    prob = Problem(mesh="cube01_hex", rs=2, order_v=3, order_e=2, problem=1)
    S = deformed_state(prob, seed=71)
    o = make_oracle(prob)
    try:
        o.cg_tol = 1e-14
        dS_o = np.empty_like(S)
        o.qdata_is_current = False
        o.mult(S, dS_o)
    finally:
        o.close()
    H1V = prob.H1V
    monkeypatch.setenv("LGH_VCG_VARIANT", "4")
    res = {}
    for merge in ("1", "0"):
        for dyn in ("1", "0"):
            monkeypatch.setenv("LGH_SLAB_MERGE", merge)
            monkeypatch.setenv("LGH_SLAB_DYN", dyn)
            g = make_gpu(prob)
            try:
                assert g.ctx.k1_form() == "slab"
                g.cg_tol = 1e-14
                Sd, dS = g.ctx.to_dev(S), g.ctx.zeros(S.size)
                g.reset_quadrature_data()
                g.mult(Sd, dS)
                g.ctx.sync()
                _, n_merged = g.ctx.test_vcg_merged_faces()
                assert (n_merged > 0) == (merge == "1")
                res[merge, dyn] = dS.cpu().numpy()[H1V:2 * H1V]
            finally:
                g.close()
            assert rel_err(res[merge, dyn], dS_o[H1V:2 * H1V]) < 1e-10
        assert np.array_equal(res[merge, "1"], res[merge, "0"]), "exact accumulation: the result must not depend on the schedule"
    assert rel_err(res["1", "1"], res["0", "1"]) < 1e-11


@pytest.mark.parametrize("tol,max_iter", [(1e-8, 300), (1e-14, 5), (1e-3, 300), (1e-8, 1)], ids=["tol1e-8", "cut-at-5", "tol1e-3", "one-iteration"])
def test_slab_cg_bookkeeping_exact_rz(tol, max_iter, monkeypatch):
    """The bookkeeping of the lockstep solve when (r, z) lives in exact accumulators (lgh_vcg.hpp, rz_limbs mode: K2 has
    no last workgroup, the next K1 folds the sums and commits `done` / `iters` / `all_done`, a one-thread kernel does it
    for the last enqueued iteration): stops by tolerance (components leave the iteration at different counts), by the
    iteration cap in the middle of the first enqueued chunk, after a single iteration, and with a loose tolerance.
    Against the oracle's solve with the same parameters, and against the ticketed reduction (LGH_RZ_LIMBS=0); a
    second evaluation on the same context (first chunk = the count the first one left) must reproduce the first."""
    from oracle.fem import Problem
    prob = Problem(mesh="box01_hex", rs=1, order_v=3, order_e=2, problem=1)
    S = deformed_state(prob, seed=61)
    H1V = prob.H1V
    o = make_oracle(prob)
    try:
        o.cg_tol, o.cg_max_iter = tol, max_iter
        dS_o = np.empty_like(S)
        o.qdata_is_current = False
        o.reset_timers()
        o.mult(S, dS_o)
        it_o = o.timers()["H1iter"]
    finally:
        o.close()
    monkeypatch.setenv("LGH_VCG_VARIANT", "4")
    its, errs = {}, {}
    for mode in ("1", "0"):
        monkeypatch.setenv("LGH_RZ_LIMBS", mode)
        g = make_gpu(prob)
        try:
            assert g.ctx.k1_form() == "slab"
            g.ctx.enable_timers(True)
            g.cg_tol, g.cg_max_iter = tol, max_iter
            Sd = g.ctx.to_dev(S)
            dS = g.ctx.zeros(S.size)
            for rep in range(2):  # (the second evaluation starts from the iteration count the first one left: a different first chunk)
                g.ctx.reset_timers()
                g.reset_quadrature_data()
                g.mult(Sd, dS)
                g.ctx.sync()
                its[mode, rep] = g.ctx.timers()["H1iter"]
                got = dS.cpu().numpy()
                errs[mode, rep] = rel_err(got[H1V:2 * H1V], dS_o[H1V:2 * H1V])
        finally:
            g.close()
    # (Iterates of differently rounded CG runs drift apart as the Ritz values converge: after 8 orders of residual
    #  reduction on this distorted random state every form of the solve - column, plane, slab, either K2 - is 3e-9 to
    #  2e-8 away from the oracle's iterate of the same index, i.e. within the distance of that iterate from the
    #  solution, and a stop one iteration apart is possible; with the cap, one iteration or a loose or tight tolerance
    #  the agreement is 1e-10.  profiles/r4_k2_tail.txt has the numbers.)
    assert its["1", 0] == its["1", 1] and its["0", 0] == its["0", 1], its
    assert max(abs(v - it_o) for v in its.values()) <= (1 if tol == 1e-8 else 0), (its, it_o, errs)
    assert max(errs.values()) < (5e-8 if tol == 1e-8 else 1e-10), (errs, its, it_o)


@pytest.mark.parametrize("variant", ["2", "4"], ids=["plane", "slab"])
def test_mass_data_forms(variant, monkeypatch):
    """Compact mass data (lgh_mass_data_form: D[q, e] = W[q] s_e, found by a device check at first use) against the
    stored table.  Sedov on a Cartesian mesh has it; after the table is rewritten through lgh_mass_D() with a factor
    that varies inside the elements the check must fail and the kernels must read the new table: H1 and L2 mass
    products and the lockstep velocity solve then agree with a run that has the compact form switched off
    (LGH_MASS_RANK1=0: same kernels, same data, hence the same bits), and differ from the products of the old data."""
    from oracle.fem import Problem
    prob = Problem(mesh="box01_hex", rs=1, order_v=3, order_e=2, problem=1)
    S = deformed_state(prob, seed=51)
    xv, xe = seeded(prob.N, 52), seeded(prob.L2V, 53)
    factor = 1.0 + 0.25 * np.abs(seeded(prob.NE * prob.NQ, 54))
    monkeypatch.setenv("LGH_VCG_VARIANT", variant)
    import torch

    def run(rewrite):
        g = make_gpu(prob)
        try:
            form0 = g.ctx.mass_data_form()
            if rewrite:
                g.ctx.massD = g.ctx.massD * factor  # (the setter calls lgh_mass_D again after the write: its contract)
            form1 = g.ctx.mass_data_form()
            yv, ye = g.ctx.empty(prob.N), g.ctx.empty(prob.L2V)
            xvd, xed, Sd = g.ctx.to_dev(xv), g.ctx.to_dev(xe), g.ctx.to_dev(S)
            torch.cuda.synchronize()
            g.ctx.mass_set_ess(-1)
            g.ctx.mass_mult(0, xvd, yv)
            g.ctx.mass_mult(1, xed, ye)
            g.cg_tol = 1e-14
            dS = g.ctx.zeros(S.size)
            g.reset_quadrature_data()
            g.mult(Sd, dS)
            g.ctx.sync()
            return form0, form1, yv.cpu().numpy(), ye.cpu().numpy(), dS.cpu().numpy()
        finally:
            g.close()

    f0, f1, yv_c, ye_c, dS_c = run(False)
    assert (f0, f1) == ("rank1", "rank1")
    f0, f1, yv_w, ye_w, dS_w = run(True)
    assert (f0, f1) == ("rank1", "stored"), "a rewritten table must be looked at again"
    monkeypatch.setenv("LGH_MASS_RANK1", "0")
    f0, f1, yv_s, ye_s, dS_s = run(True)
    assert (f0, f1) == ("stored", "stored")
    assert np.array_equal(yv_w, yv_s) and np.array_equal(ye_w, ye_s) and np.array_equal(dS_w, dS_s)
    assert rel_err(yv_w, yv_c) > 1e-3 and rel_err(ye_w, ye_c) > 1e-3
    f0, f1, yv_t, ye_t, dS_t = run(False)      # the stored table of the unmodified data against its compact form
    assert rel_err(yv_t, yv_c) < 1e-12 and rel_err(ye_t, ye_c) < 1e-12  # (the check admits 1e-12 per entry)
    H1V = prob.H1V
    assert rel_err(dS_t[H1V:], dS_c[H1V:]) < 1e-10


def test_stored_mass_table_does_not_trip_the_dt_estimate():
    """Round-4 advisor: the 'mass table is not compact' flag and the 'energy right-hand side poisoned' flag shared one
    device word, so on a context whose mass data is genuinely not W[q]*s_e (a graded mesh, a density that varies inside
    a zone) the first lgh_get_dt_est after a mass apply failed with the poisoned-velocity error.  Each flag has its own
    word now: a rewritten, truly non-compact table -> mass apply -> a whole Mult -> the dt estimate must come back."""
    from oracle.fem import Problem
    prob = Problem(mesh="box01_hex", rs=1, order_v=3, order_e=2, problem=1)
    S = deformed_state(prob, seed=61)
    factor = 1.0 + 0.25 * np.abs(seeded(prob.NE * prob.NQ, 62))
    import torch
    g = make_gpu(prob)
    try:
        g.ctx.massD = g.ctx.massD * factor
        assert g.ctx.mass_data_form() == "stored"
        xv, yv = g.ctx.to_dev(seeded(prob.N, 63)), g.ctx.empty(prob.N)
        torch.cuda.synchronize()
        g.ctx.mass_set_ess(-1)
        g.ctx.mass_mult(0, xv, yv)
        g.ctx.set_dt_est(0.125)
        assert g.ctx.get_dt_est() == 0.125          # (raised "velocity other than the state's" before the fix)
        Sd, dS = g.ctx.to_dev(S), g.ctx.zeros(S.size)
        g.reset_quadrature_data()
        g.reset_time_step_estimate()
        g.mult(Sd, dS)
        dt = g.get_time_step_estimate(Sd)
        assert np.isfinite(dt) and dt > 0
        g.ctx.mass_data_changed()                    # the check runs again (and must not erase or fake a poison report)
        g.ctx.mass_mult(0, xv, yv)
        assert g.ctx.get_dt_est() == dt
    finally:
        g.close()


@pytest.mark.parametrize("variant", ["2", "4"], ids=["plane", "slab"])
def test_mass_data_changed_keeps_operator_and_diagonal_consistent(variant, monkeypatch):
    """A caller that keeps the lgh_mass_D() pointer and rewrites the table AFTER a mass apply has run (round-3 advisor:
    the compact form would stay stale in the plane / slab kernels while the column kernels and the Jacobi diagonal
    see other data) announces it with lgh_mass_data_changed(): the form is detected again and the diagonal is
    reassembled.  A table scaled by 2 (exact in binary) must double the product, the diagonal and K1's E-vector bit
    for bit and stay compact; a factor that varies inside the elements must switch every kernel to the stored table."""
    from oracle.fem import Problem
    prob = Problem(mesh="box01_hex", rs=1, order_v=3, order_e=2, problem=1)
    monkeypatch.setenv("LGH_VCG_VARIANT", variant)
    xv = seeded(prob.N, 61)
    r = seeded(3 * prob.N, 62)
    g = make_gpu(prob)
    try:
        ctx = g.ctx
        D0 = np.array(ctx.massD, copy=True)
        diag0 = np.array(ctx.mass_diag, copy=True)
        xvd, rd = ctx.to_dev(xv), ctx.to_dev(r)
        ctx.mass_set_ess(-1)

        def products():
            y = ctx.empty(prob.N)
            ctx.mass_mult(0, xvd, y)
            ctx.sync()
            dinv = 1.0 / np.asarray(ctx.mass_diag)
            rz = np.array([float(np.dot(r[c * prob.N:(c + 1) * prob.N] ** 2, dinv)) for c in range(3)])
            yE, den = ctx.test_vcg_k1(rd, None, rz, rz, True)
            return y.cpu().numpy(), yE.cpu().numpy().copy(), den, rz

        y0, yE0, den0, rz0 = products()
        assert ctx.mass_data_form() == "rank1"
        ctx.write_massD_in_place(2.0 * D0)      # pointer kept, no lgh_mass_D() afterwards
        ctx.mass_data_changed()
        y1, yE1, den1, rz1 = products()
        assert ctx.mass_data_form() == "rank1"
        assert np.array_equal(np.asarray(ctx.mass_diag), 2.0 * diag0)
        assert np.array_equal(y1, 2.0 * y0)
        # d = r/diag halves, A doubles: the E-vector is unchanged, (d, A d) halves - exactly
        assert np.array_equal(yE1, yE0) and np.array_equal(den1, 0.5 * den0)
        factor = 1.0 + 0.25 * np.abs(seeded(prob.NE * prob.NQ, 63))
        ctx.write_massD_in_place(D0 * factor)
        ctx.mass_data_changed()
        y2, yE2, den2, rz2 = products()
        assert ctx.mass_data_form() == "stored"
        assert rel_err(y2, y0) > 1e-3
        # the preconditioner belongs to the new operator: diag = diagonal of the matrix the kernels apply
        e = np.zeros(prob.N)
        n0 = prob.N // 2
        e[n0] = 1.0
        col = ctx.empty(prob.N)
        ctx.mass_mult(0, ctx.to_dev(e), col)
        ctx.sync()
        assert abs(col.cpu().numpy()[n0] - np.asarray(ctx.mass_diag)[n0]) < 1e-13 * abs(diag0[n0])
    finally:
        g.close()


@pytest.mark.parametrize("order", [(3, 2), (4, 3)], ids=["Q3Q2", "Q4Q3"])
def test_mass_kernels_without_table_symmetry(order, monkeypatch):
    """LGH_B_SYM=0: lgh_create treats the 1-D tables as not mirror symmetric, as it would for a basis on asymmetric
    points - the lockstep K1 then keeps the whole table in scalar registers (Q3Q2) or runs in column form (Q4Q3) and
    the L2 mass apply runs in column form.  One RHS evaluation on a distorted state (both CGs to 1e-14) against the
    oracle, as for the default dispatch."""
    from oracle.fem import Problem
    prob = Problem(mesh="box01_hex", rs=0, order_v=order[0], order_e=order[1], problem=1)
    S = deformed_state(prob, seed=35)
    o = make_oracle(prob)
    try:
        o.cg_tol = 1e-14
        dS_o = np.empty_like(S)
        o.qdata_is_current = False
        o.mult(S, dS_o)
    finally:
        o.close()
    monkeypatch.setenv("LGH_B_SYM", "0")
    g = make_gpu(prob)
    try:
        assert g.ctx.table_symmetry() == (0, 0)
        g.cg_tol = 1e-14
        Sd = g.ctx.to_dev(S)
        dS = g.ctx.zeros(S.size)
        g.reset_quadrature_data()
        g.mult(Sd, dS)
        g.ctx.sync()
        dS = dS.cpu().numpy()
    finally:
        g.close()
    H1V = prob.H1V
    assert rel_err(dS[H1V:2 * H1V], dS_o[H1V:2 * H1V]) < 1e-10
    assert rel_err(dS[2 * H1V:], dS_o[2 * H1V:]) < 1e-10


# Every environment switch that selects a different kernel or launch sequence (DESIGN.md "Environment switches"), each
# with the claim that goes with it: "bits" = the state must equal the default dispatch bit for bit (same operations in
# the same order, only organised differently), "tol" = a different kernel / summation order, oracle tolerance only.
KERNEL_SWITCHES = [
    ((3, 2), {"LGH_FUSED_INIT": "0"}, "bits"),
    ((3, 2), {"LGH_OVERLAP": "0"}, "bits"),
    ((3, 2), {"LGH_K2_SKIP": "0"}, "bits"),
    ((3, 2), {"LGH_JAC0_COMPACT": "0"}, "tol"),
    ((4, 3), {"LGH_JAC0_COMPACT": "0"}, "tol"),
    ((3, 2), {"LGH_FUSED_FTV": "0"}, "tol"),
    ((3, 2), {"LGH_FUSED_F1": "0"}, "tol"),
    ((3, 2), {"LGH_FUSED_FTV": "0", "LGH_FUSED_F1": "0"}, "tol"),
    ((3, 2), {"LGH_K2P": "0"}, "tol"),
    ((3, 2), {"LGH_K2_GRID": "2"}, "tol"),
    ((3, 2), {"LGH_K2_NODE_WEIGHT": "-1"}, "tol"),
    ((3, 2), {"LGH_MASS_RANK1": "0"}, "tol"),
    ((4, 3), {"LGH_MASS_RANK1": "0"}, "tol"),
    ((3, 2), {"LGH_MASS_SEP": "0"}, "tol"),
    ((4, 3), {"LGH_MASS_SEP": "0"}, "tol"),
    ((5, 4), {"LGH_MASS_SEP": "0"}, "tol"),
    ((5, 4), {"LGH_MASS_RANK1": "0"}, "tol"),
    ((5, 4), {"LGH_Q_PPT": "1"}, "tol"),
    # mass operators through the quadrature points instead of the Kronecker form of compact data (slab K1, L2 apply)
    ((3, 2), {"LGH_MASS_KRON": "0"}, "tol"),
    ((4, 3), {"LGH_MASS_KRON": "0"}, "tol"),
    ((5, 4), {"LGH_MASS_KRON": "0"}, "tol"),
    ((3, 2), {"LGH_MASS_KRON": "0", "LGH_VCG_VARIANT": "4"}, "tol"),
    ((3, 2), {"LGH_RZ_LIMBS": "0", "LGH_VCG_VARIANT": "4"}, "tol"),  # (r, z) by the ticketed reduction of K2 instead of exact accumulators
    ((3, 2), {"LGH_Q_OCC4": "1"}, "bits"),  # the 128-register build of the row form (what contexts without viscosity get): same operations
    ((3, 2), {"LGH_Q_FORM": "0"}, "tol"),   # the point form of the quadrature update instead of the row form (lgh_qrows.hpp)
    ((4, 3), {"LGH_Q_FORM": "0"}, "tol"),
    ((3, 2), {"LGH_Q_FORM": "0", "LGH_FUSED_FTV": "0", "LGH_FUSED_F1": "0"}, "tol"),
    ((4, 3), {"LGH_L2_PLANE": "0"}, "tol"),
    ((4, 3), {"LGH_K2P": "0"}, "tol"),
    # round 6: the energy CG's update by cg_update_k on the stored M d instead of the Kronecker kernel forming it again (another
    # kernel: x and r round differently); host looks through hipStreamSynchronize instead of the token spin
    ((3, 2), {"LGH_L2_FUSED": "0"}, "tol"),
    ((4, 3), {"LGH_L2_FUSED": "0"}, "tol"),
    ((3, 2), {"LGH_SPIN": "0"}, "bits"),
    ((5, 4), {"LGH_KRON_NEB": "0"}, "tol"),  # four / eight instead of two / three zones per workgroup of the Kronecker K1
    ((4, 3), {"LGH_KRON_NEB": "0"}, "tol"),
    ((5, 4), {"LGH_L2_NEB": "0"}, "tol"),  # sixteen instead of ten zones per workgroup of the L2 Kronecker kernel (other partial sums)
]
_switch_default = {}


@pytest.mark.parametrize("order,switches,claim", KERNEL_SWITCHES,
                         ids=lambda v: ",".join(f"{k[4:]}={x}" for k, x in v.items()) if isinstance(v, dict) else (f"Q{v[0]}Q{v[1]}" if isinstance(v, tuple) else v))
def test_kernel_switches(order, switches, claim, monkeypatch):
    """No untested kernel behind an environment variable: one right-hand-side evaluation (QUpdate, both force
    products, the lockstep velocity solve, the energy solve; both CGs to 1e-14) on a distorted state with the switch
    set, against the oracle - and against the default dispatch bit for bit where the switch only reorganises the
    launches."""
    from oracle.fem import Problem
    prob = Problem(mesh="box01_hex", rs=1 if order == (3, 2) else 0, order_v=order[0], order_e=order[1], problem=1)
    S = deformed_state(prob, seed=45)
    H1V = prob.H1V

    # (order 4 Bernstein mass matrix without preconditioner: the energy CG needs more than the reference's cap of 300
    #  iterations to converge, and an iteration cut off unconverged amplifies every rounding difference - let it finish)
    max_iter = 300 if order != (5, 4) else 4000

    def run():
        g = make_gpu(prob)
        try:
            g.cg_tol, g.cg_max_iter = 1e-14, max_iter
            Sd = g.ctx.to_dev(S)
            dS = g.ctx.zeros(S.size)
            g.reset_quadrature_data()
            g.mult(Sd, dS)
            g.ctx.sync()
            return dS.cpu().numpy()
        finally:
            g.close()

    if order not in _switch_default:
        o = make_oracle(prob)
        try:
            o.cg_tol, o.cg_max_iter = 1e-14, max_iter
            dS_o = np.empty_like(S)
            o.qdata_is_current = False
            o.mult(S, dS_o)
        finally:
            o.close()
        _switch_default[order] = (dS_o, run())
    dS_o, dS_def = _switch_default[order]
    assert rel_err(dS_def[H1V:2 * H1V], dS_o[H1V:2 * H1V]) < 1e-10
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    dS = run()
    assert rel_err(dS[H1V:2 * H1V], dS_o[H1V:2 * H1V]) < 1e-10
    assert rel_err(dS[2 * H1V:], dS_o[2 * H1V:]) < (1e-10 if order != (5, 4) else 1e-8)  # (cond ~ 1e6 at order 4)
    if claim == "bits":
        assert np.array_equal(dS, dS_def)


@pytest.mark.parametrize("n", [5, 4096, 4097, 1000003])
def test_vec_axpby_pair_has_the_bits_of_two_axpbys(n):
    """lgh_vec_axpby_pair (the two combinations an RK stage forms from one increment, in one pass over it) against two
    lgh_vec_axpby calls: bit for bit, odd lengths and the in-place form z2 = z2 + b k included.  The C++ driver's RK4 uses
    the pair, the Python driver two calls: test_cpp_driver_matches_python_driver holds whole runs to the same bits."""
    from oracle.fem import Problem
    g = make_gpu(Problem(mesh="cube01_hex", rs=0, order_v=2, order_e=1, problem=1))
    try:
        S, k, zin = seeded(n, 401), seeded(n, 402), seeded(n, 403)
        Sd, kd = g.ctx.to_dev(S), g.ctx.to_dev(k)
        y1, z1 = g.ctx.empty(n), g.ctx.to_dev(zin)
        y2, z2 = g.ctx.empty(n), g.ctx.to_dev(zin)
        import torch
        torch.cuda.synchronize()
        g.ctx.vec_axpby(y1, 1.0, Sd, 0.37, kd)
        g.ctx.vec_axpby(z1, 1.0, z1, 0.11, kd)
        g.ctx.vec_axpby_pair(y2, 1.0, Sd, 0.37, z2, 1.0, z2, 0.11, kd)
        g.ctx.sync()
        assert np.array_equal(y1.cpu().numpy(), y2.cpu().numpy()) and np.array_equal(z1.cpu().numpy(), z2.cpu().numpy())
        assert np.array_equal(y1.cpu().numpy(), 1.0 * S + 0.37 * k) or rel_err(y1.cpu().numpy(), S + 0.37 * k) < 1e-15
    finally:
        g.close()
