"""The element grids of tests/shape_cases.py on the oracle alone (no GPU): what the GPU tests on these grids take for
granted is checked here, where a failure says "the case is wrong", not "the kernel is wrong".

  * every (shape, mesh, order) builds, and one right-hand side of the oracle on helpers.deformed_state is finite;
  * closed forms that owe nothing to either implementation: sum rho0 detJ0 w = rho0 * volume of the box;
    1^T M_H1 1 = 1^T M_L2 1 = the same number (both bases sum to 1); M symmetric through u.(M w) = w.(M u);
  * the iteration cap of the whole right-hand sides (tests/test_gpu_shapes_solve.py: both CGs at 1e-14, cap 4000) is a
    condition, not a tolerance: on the mesh shape_cases.solve_mesh names for the order, the oracle's CGs stop BELOW it.
    Measured with a seeded right-hand side: graded meshes need up to 120 (Q2Q1), 693 (Q3Q2), 4144 (Q4Q3) and 11 000 to
    26 000 (Q5Q4) energy iterations - every zone has its own s_e, the unpreconditioned Bernstein mass many distinct
    eigenvalues, and a CG that long amplifies rounding; equal meshes 5, 18, 48, 150."""
import numpy as np
import pytest

import shape_cases as sc
from helpers import deformed_state, make_oracle, seeded

CASES = [(c, m) for c in sc.all_cases() for m in sc.MESHES]


def test_chain_counts_follow_from_the_shape():
    """the formula against a walk over the zones that knows rows, not nodes"""
    for shape in sc.SHAPES_3D:
        nx, NE = shape[0], int(np.prod(shape))
        count = 0
        for s in range(NE // 5):
            rows = {(e // nx) for e in range(5 * s, 5 * s + 5)}
            count += len(rows) == 1
        assert count == sc.n_chains(shape), shape
    assert sc.n_merged((7, 3, 2)) == 4 * 64 and sc.n_merged((3, 3, 3)) == 0


@pytest.mark.parametrize("mesh", sc.MESHES)
@pytest.mark.parametrize("shape", list(sc.SHAPES_3D) + list(sc.SHAPES_2D), ids=sc.shape_id)
def test_breaks(shape, mesh):
    b = sc.breaks(shape, mesh)
    assert [len(x) - 1 for x in b] == list(shape)
    for a, x in enumerate(b):
        assert x[0] == 0.0 and x[-1] == sc.AXIS_LENGTHS[a] and np.all(np.diff(x) > 0)
        w = np.diff(x) * shape[a] / sc.AXIS_LENGTHS[a]
        # (equal: a difference of two break points rounded to 2^-53 each, times n <= 17 over the length: < 1e-14)
        assert np.all(np.abs(w - 1.0) <= (0.30 if mesh == "graded" else 1e-14))
    assert all(np.array_equal(x, y) for x, y in zip(b, sc.breaks(shape, mesh)))   # fixed seed


@pytest.mark.parametrize("case,mesh", CASES, ids=[f"{sc.case_id(c)}-{m}" for c, m in CASES])
def test_oracle_on_shape(case, mesh):
    shape, order = case
    prob = sc.make_problem(shape, mesh, order)    # (asserts distinct volumes and hx != hy != hz on the graded mesh)
    solve = mesh == sc.solve_mesh(order)
    o = make_oracle(prob)
    try:
        # closed forms (problem 1: rho0 = 1)
        vol = sc.box_volume(shape)
        assert abs(float(np.sum(o.rho0DetJ0w)) - vol) <= 1e-13 * vol
        # (the volume is summed from det J of the Lagrange gradient table: D1D products with |G| up to ~20 that cancel to
        #  the zone width, a few 1e-14 per point at Q4 and Q5; the mass data above has the exact widths in it)
        assert abs(o.volume - vol) <= 1e-12 * vol
        m_h1 = float(np.sum(o.mass_mult(0, np.ones(prob.N))))
        m_l2 = float(np.sum(o.mass_mult(1, np.ones(prob.L2V))))
        assert abs(m_h1 - vol) <= 1e-13 * vol and abs(m_l2 - vol) <= 1e-13 * vol
        for space, n in ((0, prob.N), (1, prob.L2V)):
            u, w = seeded(n, 401 + space), seeded(n, 403 + space)
            Mu, Mw = o.mass_mult(space, u), o.mass_mult(space, w)
            assert abs(float(u @ Mw) - float(w @ Mu)) <= 1e-13 * np.linalg.norm(u) * np.linalg.norm(Mw)
        # one right-hand side; where the GPU tests solve on this mesh: with their tolerance and cap, and below the cap
        S = deformed_state(prob)
        if solve:
            o.cg_tol, o.cg_max_iter = sc.CG_TOL, sc.CG_CAP
        dS = np.empty_like(S)
        o.qdata_is_current = False
        o.reset_timers()
        o.mult(S, dS)
        assert np.all(np.isfinite(dS))
        if solve:
            t = o.timers()
            print(f"{sc.case_id(case)} {mesh}: H1 iterations (3 components) {t['H1iter']}, L2 iterations {t['L2iter']}")
            assert t["L2iter"] < sc.CG_CAP and t["H1iter"] < sc.CG_CAP
            # ... and for a seeded right-hand side of the energy solve alone
            _, it = o.cg(1, seeded(prob.L2V, 13), rel_tol=sc.CG_TOL, max_iter=sc.CG_CAP)
            assert it < sc.CG_CAP, it
    finally:
        o.close()


def test_problem_0_builds_on_7x3x2():
    """the instantiation without viscosity runs on one 3D shape (Taylor-Green has no source at the origin)"""
    prob = sc.make_problem((7, 3, 2), "graded", (3, 2), problem=0)
    o = make_oracle(prob)
    try:
        S = deformed_state(prob)
        dS = np.empty_like(S)
        o.qdata_is_current = False
        o.mult(S, dS)
        assert np.all(np.isfinite(dS)) and not prob.use_viscosity()
    finally:
        o.close()
