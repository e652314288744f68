"""The routes one lgh_solve_velocity call can take agree (lgh_velocity.hip).

3D (cube01_hex rs=1 Q2Q1, problem 1: the lockstep CG).  With the region timers off the right-hand side is formed inside the
first kernel of the CG (fused-init), with them on by separate kernels; F.1 comes from the fused quadrature update or from the
force kernel; `one` is NULL (the operator's own) or a vector whose content is checked.  For a fixed source of F.1 the four
combinations of timers and `one` give the same bits in dv, rhs_h1 and the iteration count; across the two sources dv agrees to
the operator tolerance (the fused update sums in its own order: no bit equality is claimed); a vector that is not all ones
goes through the force kernel.

2D (rt2D rs=1 Q3Q2, problem 7: one scalar CG per component, the gravity source).  Timers on and off give the same bits, rhs_h1
comes back with an exact 0.0 at every essential dof of every component - the scalar CG is handed a copy of it and relies on
that - and dv matches the oracle.

CG tolerance 1e-14, at most 300 iterations; one context per mesh, shared by the tests of the module."""
import numpy as np
import pytest

from helpers import deformed_state, make_gpu, make_oracle, rel_err

pytestmark = pytest.mark.gpu

TOL, CAP = 1e-14, 300


class _Case:
    """one context, one oracle, one deformed state with its quadrature data on both sides"""

    def __init__(self, prob, seed):
        self.prob = prob
        self.g, self.o = make_gpu(prob, cg_tol=TOL, cg_max_iter=CAP), make_oracle(prob, cg_tol=TOL, cg_max_iter=CAP)
        self.Sh = deformed_state(prob, seed=seed)
        self.S = self.g.ctx.to_dev(self.Sh)
        self.dS, self.rhs, self.work = self.g.ctx.zeros(self.Sh.size), self.g.ctx.zeros(prob.H1V), self.g.ctx.zeros(prob.N)
        self.qupdate()

    def qupdate(self):
        self.g.reset_quadrature_data()
        self.g.update_quadrature_data(self.S)

    def solve(self, timers, one=None):
        """(dv, rhs_h1, iterations) of one lgh_solve_velocity; both output vectors start from a pattern no route leaves behind"""
        import torch
        ctx, H1V = self.g.ctx, self.prob.H1V
        ctx.enable_timers(timers)
        self.dS.fill_(7.0)
        self.rhs.fill_(-3.0)
        torch.cuda.synchronize()
        its = ctx.solve_velocity(self.S, self.dS, one, self.rhs, self.work, TOL, CAP)
        ctx.sync()
        return self.dS[H1V:2 * H1V].cpu().numpy().copy(), self.rhs.cpu().numpy().copy(), its

    def close(self):
        self.g.ctx.enable_timers(True)
        self.g.close()
        self.o.close()


@pytest.fixture(scope="module")
def cube():
    from oracle.fem import Problem
    case = _Case(Problem(mesh="cube01_hex", rs=1, order_v=2, order_e=1, problem=1), seed=43)
    yield case
    case.close()


@pytest.fixture(scope="module")
def rt():
    from oracle.fem import Problem
    case = _Case(Problem(mesh="rt2D", rs=1, order_v=3, order_e=2, problem=7), seed=3)
    yield case
    case.close()


def _same_bits(a, b, what):
    assert np.array_equal(a[0], b[0]), f"dv differs, {what}: rel {rel_err(a[0], b[0]):.3e}"
    assert np.array_equal(a[1], b[1]), f"rhs_h1 differs, {what}: rel {rel_err(a[1], b[1]):.3e}"
    assert a[2] == b[2], f"iteration count differs, {what}: {a[2]} vs {b[2]}"


def _routes_3d(case):
    """the four combinations of timers and `one` for the F.1 source the context has now; returns the first"""
    ones = case.g.ctx.to_dev(np.ones(case.prob.L2V))
    first = case.solve(timers=False)
    assert 0 < first[2] < 3 * CAP and np.isfinite(first[0]).all()
    _same_bits(first, case.solve(timers=True), "timers off (fused-init) against timers on (separate kernels)")
    _same_bits(first, case.solve(timers=False, one=ones), "one = NULL against explicit ones, timers off")
    _same_bits(first, case.solve(timers=True, one=ones), "one = NULL against explicit ones, timers on")
    return first


def test_3d_routes_agree_for_either_source_of_f1(cube):
    assert cube.g.ctx.k1_form() is not None, "the shape is meant to have the lockstep solve"
    try:
        cube.g.ctx.set_fused_forces(True)
        cube.qupdate()
        assert cube.g.ctx.quadrature_generation()[1] == 1, "F.1 of the fused update is meant to be on hand"
        fused = _routes_3d(cube)
        cube.g.ctx.set_fused_forces(False)
        cube.qupdate()
        assert cube.g.ctx.quadrature_generation()[1] == 0, "the force kernel is meant to run"
        kernel = _routes_3d(cube)
    finally:
        cube.g.ctx.set_fused_forces(True)
        cube.qupdate()
    e = rel_err(fused[0], kernel[0])
    print(f"dv, fused update against force kernel: rel {e:.3e}")
    assert e < 1e-10


@pytest.mark.parametrize("timers", [False, True], ids=["timers-off", "timers-on"])
def test_3d_vector_that_is_not_all_ones_takes_the_force_kernel(cube, timers):
    x = np.ones(cube.prob.L2V)
    x[::7] = 0.5
    cube.o.qdata_is_current = False
    cube.o.update_quadrature_data(cube.Sh)
    ref = cube.o.force_mult(x)
    assert rel_err(ref, cube.o.force_mult(np.ones(cube.prob.L2V))) > 1e-3  # far from F.1
    _, r, _ = cube.solve(timers=timers, one=cube.g.ctx.to_dev(x))
    free = r != 0.0  # rhs_h1 holds -F x with the essential rows zeroed; compare away from them
    assert free.sum() > r.size // 2
    assert rel_err(-r[free], ref[free]) < 1e-12


def test_2d_scalar_route_timers_and_eliminated_rhs(rt):
    prob = rt.prob
    assert rt.g.ctx.k1_form() is None, "the shape is meant to have no lockstep solve"
    off = rt.solve(timers=False)
    on = rt.solve(timers=True)
    _same_bits(off, on, "timers off against timers on")
    assert 0 < off[2] < prob.dim * CAP
    for comp in range(prob.dim):
        ess = np.asarray(prob.ess[comp], dtype=np.int64)
        assert ess.size > 0
        at_ess = off[1][comp * prob.N + ess]
        assert np.array_equal(at_ess, np.zeros(ess.size)), f"rhs_h1 of component {comp} is not 0.0 at every essential dof"
    assert np.abs(off[1]).max() > 0.0
    dS_o = np.empty_like(rt.Sh)
    rt.o.qdata_is_current = False
    rt.o.mult(rt.Sh, dS_o)
    e = rel_err(off[0], dS_o[prob.H1V:2 * prob.H1V])
    print(f"dv against the oracle: rel {e:.3e}")
    assert e < 1e-10
