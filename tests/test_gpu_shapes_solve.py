"""The kernels together on element grids that are not powers of two (tests/shape_cases.py; the operators one by one:
tests/test_gpu_shapes_operators.py).

  * one right-hand side (quadrature update, force products, the lockstep velocity solve, the energy solve; both CGs at
    1e-14 with a cap of 4000 that tests/test_shape_cases.py shows the oracle stays below) on helpers.deformed_state, for
    every (shape, order) in the default dispatch and at Q3Q2 with every form of K1 forced - where K1's E-vector layout
    and K2's tables have to agree on sets that are ragged, straddle rows of zones or are no chains at all.  Graded mesh
    up to Q3Q2, equal mesh at Q4Q3 and Q5Q4 (shape_cases.solve_mesh).  Bars of test_hydro_mult and
    tests/test_gpu_qupdate_edges.py: dx/dt 1e-13, dv/dt and de/dt 1e-10 (de/dt 1e-8 at Q5Q4);
  * six RK4 steps from t = 0 with the real dt controller against oracle.driver.run (test_gpu_configs._state_parity);
  * the same right-hand side under a random renumbering of nodes and zones (helpers.PermutedProblem), in the library's
    own order and in the caller's;
  * the C++ driver's own set-up of such grids (-nx -ny -nz -Sx -Sy -Sz) against the oracle on the same break points.
Several ranks on such grids: tests/test_gpu_ranks_3d.py holds every entry of the right-hand side to the oracle (3D; 2D:
tests/test_gpu_ranks_2d.py); whole runs are cases of tests/test_gpu_pipeline.py::test_multi_rank_run_on_one_gpu.

Measured on an MI355X, worst over the shapes and forms (two runs): dx/dt exact; dv/dt 1.8e-15 (Q1Q0), 9.4e-15 (Q2Q1),
4.7e-14 (Q3Q2), 8.3e-14 (Q4Q3), 5.7e-14 (Q5Q4) against 1e-10; de/dt 1.3e-15, 1.4e-14, 1.1e-13, 1.0e-13 against 1e-10 and
2.7e-13 (Q5Q4) against 1e-8.  The device's energy CG needs at most 19, 97, 523 (graded) and 47, 137 (equal) iterations, the
three velocity solves together at most 125: far below the cap of 4000.  The module takes 5 s."""
import numpy as np
import pytest

import shape_cases as sc
from helpers import PermutedProblem, deformed_state, make_gpu, make_oracle, rel_err
from test_gpu_configs import _state_parity

pytestmark = pytest.mark.gpu

SWITCHES = ("LGH_VCG_VARIANT", "LGH_SLAB_MERGE", "LGH_ORDER", "LGH_MASS_RANK1", "LGH_MASS_KRON")
K1_ENVS_Q3Q2 = [({"LGH_VCG_VARIANT": "0"}, "column"), ({"LGH_VCG_VARIANT": "2"}, "plane"), ({"LGH_VCG_VARIANT": "4"}, "slab"),
                ({"LGH_VCG_VARIANT": "5"}, "kron"), ({"LGH_VCG_VARIANT": "4", "LGH_SLAB_MERGE": "0"}, "slab")]
RHS_CASES = ([(c, {}, None) for c in sc.all_cases()]
             + [((s, (3, 2)), e, f) for s in sc.SHAPES_3D for e, f in K1_ENVS_Q3Q2])


def _env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _env_id(env):
    return ",".join(f"{k[4:]}={v}" for k, v in env.items()) or "default"


_oracle_rhs = {}


def oracle_rhs(case):
    """(problem, state, dS/dt of the oracle) of a (shape, order), computed once and shared by the forms; never modified"""
    if case not in _oracle_rhs:
        shape, order = case
        prob = sc.make_problem(shape, sc.solve_mesh(order), order)
        S = deformed_state(prob, seed=21)
        o = make_oracle(prob, cg_tol=sc.CG_TOL, cg_max_iter=sc.CG_CAP)
        try:
            dS_o = np.empty_like(S)
            o.qdata_is_current = False
            o.reset_timers()
            o.mult(S, dS_o)
            t = o.timers()
            assert t["L2iter"] < sc.CG_CAP and t["H1iter"] < sc.CG_CAP   # (the condition of tests/test_shape_cases.py, on this state)
        finally:
            o.close()
        S.setflags(write=False)
        dS_o.setflags(write=False)
        _oracle_rhs[case] = (prob, S, dS_o)
    return _oracle_rhs[case]


@pytest.mark.parametrize("case,env,form", RHS_CASES, ids=[f"{sc.case_id(c)}-{_env_id(e)}" for c, e, f in RHS_CASES])
def test_rhs(case, env, form, monkeypatch):
    import torch
    shape, order = case
    prob, S, dS_o = oracle_rhs(case)
    _env(monkeypatch, env)
    g = make_gpu(prob, cg_tol=sc.CG_TOL, cg_max_iter=sc.CG_CAP)
    try:
        if form is not None:
            assert g.ctx.k1_form() == form
            if form == "slab":
                want = 0 if "LGH_SLAB_MERGE" in env else sc.n_merged(shape)
                assert g.ctx.test_vcg_merged_faces()[1] == want
        g.ctx.enable_timers(True)   # (the iteration counts below)
        g.ctx.reset_timers()
        Sd = g.ctx.to_dev(np.array(S))   # (a writable copy: the shared state stays read-only)
        dS = g.ctx.zeros(S.size)
        torch.cuda.synchronize()
        g.reset_quadrature_data()
        g.mult(Sd, dS)
        g.ctx.sync()
        t = g.ctx.timers()
        dS = dS.cpu().numpy()
    finally:
        g.close()
    H1V = prob.H1V
    fig = (rel_err(dS[:H1V], dS_o[:H1V]), rel_err(dS[H1V:2 * H1V], dS_o[H1V:2 * H1V]), rel_err(dS[2 * H1V:], dS_o[2 * H1V:]))
    print(f"FIG rhs-{sc.order_id(order)} {sc.case_id(case)} {_env_id(env)}: dx {fig[0]:.2e} dv {fig[1]:.2e} de {fig[2]:.2e} H1 iterations {t['H1iter']} L2 {t['L2iter']}")
    assert np.all(np.isfinite(dS))
    assert t["H1iter"] < sc.CG_CAP and t["L2iter"] < sc.CG_CAP   # the device's CGs stopped by their tolerance too
    assert fig[0] < 1e-13
    assert fig[1] < 1e-10
    assert fig[2] < (1e-8 if order == (5, 4) else 1e-10)


# ---- six RK4 steps from t = 0 with the real dt controller ----------------------------------------------------------------
STEP_CASES = [((6, 1, 1), None), ((6, 1, 1), "4"), ((7, 3, 2), None), ((7, 3, 2), "4"), ((11, 2, 1), None), ((11, 2, 1), "4"),
              ((7, 3), None)]   # (2D has no slab form: the default dispatch only)


@pytest.mark.parametrize("shape,variant", STEP_CASES, ids=[f"{sc.shape_id(s)}-{'slab' if v else 'default'}" for s, v in STEP_CASES])
def test_six_steps(shape, variant, monkeypatch):
    """Problem 1, Q3Q2, equal mesh: same accepted and repeated steps as the oracle's run, |e| and the state to the bar of
    tests/test_gpu_configs.py::_state_parity"""
    _env(monkeypatch, {"LGH_VCG_VARIANT": variant} if variant else {})
    kw = dict(breaks=sc.breaks(shape, "equal"), order_v=3, order_e=2, problem=1)
    if variant:
        g = make_gpu(sc.make_problem(shape, "equal", (3, 2)))
        try:
            assert g.ctx.k1_form() == "slab" and g.ctx.test_vcg_merged_faces()[1] == sc.n_merged(shape)
        finally:
            g.close()
    r = _state_parity(kw, 6)
    assert r["steps"] >= 6


# ---- other numberings ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["own", "callers"])
@pytest.mark.parametrize("variant", [None, "4"], ids=["default", "slab"])
@pytest.mark.parametrize("shape", [(7, 3, 2), (11, 2, 1)], ids=sc.shape_id)
def test_rhs_on_a_permuted_mesh(shape, variant, order, monkeypatch):
    """Graded mesh, Q3Q2, random renumbering of nodes and zones: dS/dt against the oracle on the same permuted problem and
    against the structured mesh through the permutation, in the library's own order (which must find the same chains as
    on the structured mesh: sc.n_merged) and in the caller's (LGH_ORDER=0: no chain survives) - as
    tests/test_gpu_general_numbering.py does on the 512-zone cube, with the iteration cap of this module."""
    _env(monkeypatch, ({"LGH_VCG_VARIANT": variant} if variant else {}) | ({"LGH_ORDER": "0"} if order == "callers" else {}))
    base = sc.make_problem(shape, "graded", (3, 2))
    perm = PermutedProblem(base, seed=11)
    S_b = deformed_state(base, seed=23)
    S_p = perm.state(S_b)
    H1V = base.H1V

    def rhs_gpu(prob, S):
        g = make_gpu(prob, cg_tol=1e-13, cg_max_iter=sc.CG_CAP)
        try:
            form = g.ctx.k1_form()
            mo = g.ctx.mesh_order()
            assert mo["identity"] == (prob is base or order == "callers"), mo
            _, n_merged = g.ctx.test_vcg_merged_faces()
            Sd, dS = g.ctx.to_dev(S), g.ctx.zeros(S.size)
            g.reset_quadrature_data()
            g.reset_time_step_estimate()
            g.mult(Sd, dS)
            dt = g.get_time_step_estimate(Sd)
            g.ctx.sync()
            return dS.cpu().numpy(), dt, form, n_merged
        finally:
            g.close()

    dS_p, dt_p, form_p, merged_p = rhs_gpu(perm, S_p)
    dS_b, dt_b, form_b, merged_b = rhs_gpu(base, S_b)
    assert form_p == form_b
    if variant == "4":
        assert form_p == "slab" and merged_b == sc.n_merged(shape) and merged_p == (merged_b if order == "own" else 0)
    o = make_oracle(perm, cg_tol=1e-13, cg_max_iter=sc.CG_CAP)
    try:
        dS_o = np.empty_like(S_p)
        o.qdata_is_current = False
        o.reset_time_step_estimate()
        o.mult(S_p, dS_o)
        dt_o = o.get_time_step_estimate(S_p)
    finally:
        o.close()
    for name, sl in (("dv", slice(H1V, 2 * H1V)), ("de", slice(2 * H1V, None))):
        assert rel_err(dS_p[sl], dS_o[sl]) < 1e-9, (name, "vs the oracle on the permuted mesh")
        assert rel_err(dS_p[sl], perm.state(dS_b)[sl]) < 1e-9, (name, "vs the structured mesh")
    assert np.array_equal(dS_p[:H1V], S_p[H1V:2 * H1V])  # dx/dt = v
    assert abs(dt_p - dt_o) <= 1e-12 * dt_o and abs(dt_p - dt_b) <= 1e-12 * dt_b


# ---- the C++ driver's own set-up ----------------------------------------------------------------------------------------------
DRIVER_CASES = [
    ("3D-7x3x2", ["-dim", 3, "-nx", 7, "-ny", 3, "-nz", 2, "-Sx", 1, "-Sy", 1.25, "-Sz", 1.5], (7, 3, 2), (1.0, 1.25, 1.5)),
    ("2D-13x2", ["-dim", 2, "-nx", 13, "-ny", 2], (13, 2), (1.0, 1.0)),
]


@pytest.mark.parametrize("name,mesh_args,n,lengths", DRIVER_CASES, ids=[c[0] for c in DRIVER_CASES])
def test_cpp_driver_on_its_own_grid(name, mesh_args, n, lengths):
    """The driver's -Sx / -Sy / -Sz are the lengths of the box, cut into -nx / -ny / -nz equal zones (break i at S i / n):
    its initial node positions must be those of Problem(breaks=...) on these breaks - then six steps of Q3Q2 Sedov against
    the oracle's run on the same breaks: same accepted and repeated steps, dt, |e| and the state."""
    from laghos_amd import host_lib
    from oracle.driver import run as orun
    from oracle.fem import Problem
    brk = [np.array([lengths[a] * i / n[a] for i in range(n[a] + 1)]) for a in range(len(n))]
    prob = Problem(breaks=brk, order_v=3, order_e=2, problem=1)
    sim = host_lib.Sim(["-p", 1] + mesh_args + ["-rs", 0, "-ok", 3, "-ot", 2, "-pa", "-tf", 1e9, "-ms", 6, "-vs", 10 ** 9, "-cgt", 1e-12,
                        "-q"])
    try:
        sz = sim.sizes()
        assert (sz["dim"], sz["NE"], sz["N"]) == (prob.dim, prob.NE, prob.N)
        S0 = prob.initial_state()[0]
        assert rel_err(sim.state()[:prob.H1V], S0[:prob.H1V]) < 1e-14   # the same mesh, node for node
        while sim.step() == 1:
            pass
        sim.sync()
        got = dict(steps=sim.rk_steps, repeats=sim.repeats, dt=sim.dt, t=sim.t, e=sim.e_norm(), S=sim.state())
    finally:
        sim.close()
    o = orun(prob, t_final=1e9, max_steps=6, vis_steps=10 ** 9, cg_tol=1e-12)
    assert (got["steps"], got["repeats"]) == (o["steps"], o["repeats"])
    assert abs(got["t"] - o["last"]["t"]) <= 1e-11 * got["t"] and abs(got["dt"] - o["last"]["dt"]) <= 1e-10 * got["dt"]
    e_o = float(np.sqrt(np.sum(o["S"][2 * prob.H1V:] ** 2)))
    assert abs(got["e"] - e_o) / e_o < 1e-9
    assert rel_err(got["S"], o["S"]) < 1e-8
