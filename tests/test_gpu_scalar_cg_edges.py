"""The scalar CG (lgh_scg.hip: one run object, scg_begin / scg_enqueue / scg_finish) and the energy solve written on it
(lgh_energy.hip) at their edges: an iteration cap that bites, a right-hand side of zero, a non-zero start, a solve ended that was
never begun - and the three ways an energy solve runs on one rank (overlapped on the second stream, deferred to
lgh_solve_energy_end, plain lgh_solve_energy), which must agree in every bit.

Shapes: 8 hexes at Q3Q2 (Kronecker L2 apply with the fused update; the same with LGH_L2_FUSED=0: stored product, cg_update_k)
and 16 quads at Q2Q1 (column-form L2 apply, valence-4 gather).  Tolerances on solutions and iteration counts are those of
test_gpu_kernels.py::test_cg_h1 / test_cg_l2; capped and empty solves are held to their exact counts."""
import ctypes

import numpy as np
import pytest

from helpers import deformed_state, make_gpu, make_oracle, rel_err, seeded

pytestmark = pytest.mark.gpu

SHAPES = [
    ("cube01_hex", 1, 3, 2, {}),
    ("cube01_hex", 1, 3, 2, {"LGH_L2_FUSED": "0"}),
    ("square01_quad", 2, 2, 1, {}),
]
IDS = ["hex-fused", "hex-stored", "quad"]
ENERGY_CAPS = (300, 300, 3, 300, 1)


@pytest.fixture(scope="module")
def oracles():
    """one oracle per discrete problem, shared by the shapes that differ in the library's switches only"""
    from oracle.fem import Problem
    made = {}

    def get(mesh, rs, ok, ot):
        key = (mesh, rs, ok, ot)
        if key not in made:
            prob = Problem(mesh=mesh, rs=rs, order_v=ok, order_e=ot, problem=1)
            made[key] = (prob, make_oracle(prob))
        return made[key]
    yield get
    for _, o in made.values():
        o.close()


@pytest.fixture(scope="module")
def shapes(oracles):
    """shape index -> (problem, GPU operator, oracle); a context is made at its first use and lives to the end of the module"""
    made = {}

    def get(i):
        from laghos_amd import _lib
        if i not in made:
            mesh, rs, ok, ot, env = SHAPES[i]
            prob, o = oracles(mesh, rs, ok, ot)
            with pytest.MonkeyPatch.context() as mp:  # (a context's switches are those of the environment at its creation)
                for k, v in env.items():
                    mp.setenv(k, v)
                g = make_gpu(prob)
            form, compact = ctypes.c_int(-1), ctypes.c_int(-1)
            _lib.check(g.ctx.lib.lgh_l2_mass_form(g.ctx.h, ctypes.byref(form), ctypes.byref(compact)))
            assert form.value == (2 if prob.dim == 3 else 0)  # (Kronecker / column form of the L2 apply)
            made[i] = (prob, g, o)
        return made[i]
    yield get
    for _, g, _ in made.values():
        g.close()


every_shape = pytest.mark.parametrize("shape", [0, 1, 2], ids=IDS)
shapes_3d = pytest.mark.parametrize("shape", [0, 1], ids=IDS[:2])  # (the overlapped energy solve needs the lockstep velocity solve: 3D)


def rhs(prob, space):
    """(b, comp) as test_cg_h1 / test_cg_l2 set them up"""
    if space == 1:
        return seeded(prob.L2V, 13), -1
    b, comp = seeded(prob.N, 12), 1
    if len(prob.ess[comp]):
        b[prob.ess[comp]] = 0.0
    return b, comp


def gpu_cg(g, space, comp, b, x0, rel_tol, max_iter):
    import torch
    x = g.ctx.to_dev(x0)
    g.ctx.mass_set_ess(comp)
    torch.cuda.synchronize()
    it = g.ctx.cg_solve(space, g.ctx.to_dev(b), x, rel_tol, max_iter)
    g.ctx.sync()
    return x.cpu().numpy(), it


def check_full_solve(prob, g, o, space, x0=None):
    """a solve to 1e-10, held as test_cg_h1 / test_cg_l2 hold theirs"""
    b, comp = rhs(prob, space)
    x0 = np.zeros_like(b) if x0 is None else x0
    x_o, it_o = o.cg(space, b, x=x0.copy(), comp=comp, rel_tol=1e-10, max_iter=300)
    x, it = gpu_cg(g, space, comp, b, x0, 1e-10, 300)
    print(f"full solve, space {space}: {it} iterations (oracle {it_o}), rel. error {rel_err(x, x_o):.3e}")
    assert abs(it - it_o) <= (1 if space == 0 else max(1, it_o // 10)), (it, it_o)
    assert rel_err(x, x_o) < 1e-8


@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("space", [0, 1], ids=["h1", "l2"])
@every_shape
def test_iteration_cap(shapes, shape, space, m):
    """rel_tol = 0 and max_iter = m: exactly m iterations, the iterate of the oracle's m-th; the solve after it on the same
    context neither starts from a stale run nor keeps the capped count as anything but its first chunk."""
    prob, g, o = shapes(shape)
    b, comp = rhs(prob, space)
    x_o, it_o = o.cg(space, b, x=np.zeros_like(b), comp=comp, rel_tol=0.0, max_iter=m)
    assert it_o == m
    x, it = gpu_cg(g, space, comp, b, np.zeros_like(b), 0.0, m)
    print(f"cap {m}, space {space}: {it} iterations, rel. error {rel_err(x, x_o):.3e}")
    assert it == m
    assert rel_err(x, x_o) < 1e-8
    check_full_solve(prob, g, o, space)


@pytest.mark.parametrize("space", [0, 1], ids=["h1", "l2"])
@every_shape
def test_zero_right_hand_side(shapes, shape, space):
    prob, g, o = shapes(shape)
    b, comp = rhs(prob, space)
    b[:] = 0.0
    x_o, it_o = o.cg(space, b, x=np.zeros_like(b), comp=comp, rel_tol=1e-10, max_iter=300)
    assert it_o == 0
    # (the L2 solve sets x = 0 itself: hand it something else)
    x0 = np.zeros_like(b) if space == 0 else seeded(b.size, 14)
    x, it = gpu_cg(g, space, comp, b, x0, 1e-10, 300)
    assert it == 0
    assert np.all(x == 0.0)


@every_shape
def test_nonzero_start_in_h1(shapes, shape):
    """iterative mode: r = b - A x0 (cg_init_k<true> with a product that is not zero)"""
    prob, g, o = shapes(shape)
    x0 = seeded(prob.N, 15)
    if len(prob.ess[1]):
        x0[prob.ess[1]] = 0.0  # (the start satisfies the boundary condition, as dv_dt does in the application)
    check_full_solve(prob, g, o, 0, x0=x0)


def energy_solves(prob, g, S, mode):
    """dS and the iteration count of the energy solve for every cap of ENERGY_CAPS; mode: overlapped / deferred / plain"""
    ctx, H1V = g.ctx, prob.H1V
    ctx.enable_timers(mode != "overlapped")  # (region timers have sequential semantics: no overlap)
    try:
        Sd, dS = ctx.to_dev(S), ctx.zeros(S.size)
        out = []
        for e_cap in ENERGY_CAPS:
            ctx.vec_copy(dS[:H1V], Sd[H1V:2 * H1V])
            g.reset_quadrature_data()
            g.update_quadrature_data(Sd)
            if mode == "plain":
                ctx.solve_velocity(Sd, dS, None, g.rhs, g.work, 1e-14, 300)
                it = ctx.solve_energy(Sd, Sd[H1V:2 * H1V], dS, g.e_rhs, 1e-14, e_cap)
            else:
                ctx.solve_energy_begin(Sd, Sd[H1V:2 * H1V], dS, g.e_rhs, 1e-14, e_cap)
                ctx.solve_velocity(Sd, dS, None, g.rhs, g.work, 1e-14, 300)
                it = ctx.solve_energy_end()
            ctx.sync()
            out.append((dS.cpu().numpy().copy(), it))
        return out
    finally:
        ctx.enable_timers(True)


@shapes_3d
def test_three_modes_one_answer(shapes, shape):
    prob, g, o = shapes(shape)
    S = deformed_state(prob, seed=5)
    res = {mode: energy_solves(prob, g, S, mode) for mode in ("overlapped", "deferred", "plain")}
    for k, cap in enumerate(ENERGY_CAPS):
        its = [res[mode][k][1] for mode in res]
        print(f"cap {cap}: iterations {its}")
        assert its[0] == its[1] == its[2] and 1 <= its[0] <= cap
        assert np.array_equal(res["overlapped"][k][0], res["deferred"][k][0]), cap
        assert np.array_equal(res["overlapped"][k][0], res["plain"][k][0]), cap
    assert [res["plain"][k][1] for k in (2, 4)] == [3, 1]  # (the caps that bite)


@shapes_3d
def test_zero_velocity_no_source(shapes, shape):
    """e_rhs = F^T 0 = 0: the solve takes no iteration and is counted as one (laghos_solver.cpp:486)"""
    prob, g, o = shapes(shape)
    S = deformed_state(prob, seed=5)
    S[prob.H1V:2 * prob.H1V] = 0.0
    for mode in ("overlapped", "deferred"):
        for dS, it in energy_solves(prob, g, S, mode)[:2]:
            assert it == 1, mode
            assert np.all(dS[2 * prob.H1V:] == 0.0), mode


@every_shape
def test_end_without_begin(shapes, shape):
    from laghos_amd._lib import LghError
    prob, g, o = shapes(shape)
    with pytest.raises(LghError, match="laghos_hip error 1: bad argument"):
        g.ctx.solve_energy_end()
    check_full_solve(prob, g, o, 1)
    if prob.dim == 3:
        S = deformed_state(prob, seed=5)
        a, b = energy_solves(prob, g, S, "overlapped")[0], energy_solves(prob, g, S, "plain")[0]
        assert a[1] == b[1] and np.array_equal(a[0], b[0])
