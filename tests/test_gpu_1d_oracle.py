"""The 1D GPU path (lgh_1d.hip) against the oracle's full-assembly branch (oracle/laghos_oracle.cpp, "FA branch"), both
driven from the same oracle.fem.Problem.

The oracle restates the FA branch from the reference source and is pinned to README run 5 (tests/test_oracle_golden.py);
test_gpu_1d.py compares the kernels with a numpy restatement at 16 zones.  Here the sizes are the ones where the kernels'
own structure changes: one zone (every node essential at Q1Q0), two zones, 255 / 256 / 257 zones at Q1Q0 (N = 256 / 257 /
258: the first strided pass of the one-workgroup velocity CG), 257 zones at every order pair (two workgroups in every
grid reduction) and 1000 zones at Q5Q4 (four workgroups, N = 5001).  Tolerances are the 2D/3D suite's:
1e-13 of the largest entry for the linear operators and the set-up, 1e-12 for the quadrature update, dt_est and the
zone-local solve (LU inverse here, Cholesky factors there), 1e-10 for a right-hand side with both solves at -cgt 1e-14,
the _state_parity rules of test_gpu_configs.py for whole runs.

What is computed from the Jacobian J = sum_d G(q,d) x_d (set-up data, quadrature data, density) carries the round-off
of that sum, which grows with the mesh: x is O(1) while J is O(h / order).  Those quantities are held to the larger of
the base tolerance and 2 eps kappa, kappa = max over the points of sum_d |G(q,d) x_d| / |J| (jac_cond: 1 to 13 up to
two zones, 550 at 257 zones of Q1Q0, 7e4 at 1000 zones of Q5Q4, where the two sides differ by 2.6e-12 ~ eps kappa / 6).
The linear operators get the same mass and stress data on both sides and stay at 1e-13."""
import os
import subprocess

import numpy as np
import pytest

from helpers import CurvedInitialMesh, deformed_state, rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(1, 0), (2, 1), (3, 2), (4, 3), (5, 4)]
OP_CASES = [(1, 1, 0), (2, 1, 0), (2, 2, 1), (255, 1, 0), (256, 1, 0), (257, 1, 0)] + \
           [(257, a, b) for a, b in PAIRS[1:]] + [(1000, 5, 4)]


EPS = np.finfo(float).eps


def jac_cond(prob, *states):
    """kappa of the Jacobian sums at the quadrature points of the meshes in `states` (state vectors or positions)."""
    m = np.asarray(prob.h1map).reshape(prob.NE, prob.ND)
    k = 1.0
    for S in states:
        xe = np.asarray(S)[:prob.N][m]
        k = max(k, float(np.max((np.abs(xe) @ np.abs(prob.G).T) / np.abs(xe @ prob.G.T))))
    return k


def tol_j(base, prob, *states):
    return max(base, 2 * EPS * jac_cond(prob, *states))


def problem_1d(ne, ok, ot, problem=2, curved=True, E0=1.0):
    from oracle.fem import Problem
    p = Problem(breaks=[np.linspace(0.0, 1.0, ne + 1)], order_v=ok, order_e=ot, problem=problem, blast_energy=E0)
    return CurvedInitialMesh(p) if curved else p


@pytest.fixture(scope="module", params=OP_CASES, ids=[f"NE{n}-Q{a}Q{b}" for n, a, b in OP_CASES])
def pair(request):
    from helpers import make_gpu, make_oracle
    prob = problem_1d(*request.param)
    g, o = make_gpu(prob, cg_tol=1e-14, cg_max_iter=2000), make_oracle(prob, cg_tol=1e-14, cg_max_iter=2000)
    yield prob, g, o
    g.close()
    o.close()


def to_host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def test_setup(pair):
    """Jac0inv, rho0DetJ0w, the mass data, the volume, h0 and the Jacobi diagonal (laghos_solver.cpp:203-262)."""
    prob, g, o = pair
    tol = tol_j(1e-13, prob, prob.initial_state()[0])
    for got, want in ((g.ctx.Jac0inv, o.Jac0inv), (g.ctx.rho0DetJ0w, o.rho0DetJ0w), (g.ctx.massD, o.massD),
                      (g.ctx.mass_diag, o.diagV)):
        assert rel_err(got, want) <= tol
    # (the oracle sums the zone lengths; the GPU sums w detJ over the points, as GetElementVolume integrates)
    assert abs(g.volume - o.volume) <= tol * o.volume and abs(o.volume - 1.0) <= 1e-13
    assert abs(g.h0 - o.h0) <= tol * o.h0


def test_mass_and_local_solve(pair):
    """H1 mass with and without the eliminated rows, L2 mass, and x = Me(z)^-1 b zone by zone, from the same mass data
    (the oracle's, written into the context; lgh_mass_data_changed refreshes the diagonal and the zone factors)."""
    prob, g, o = pair
    ctx, rng = g.ctx, np.random.default_rng(11)
    ctx.massD = np.array(o.massD)
    ctx.mass_data_changed()
    assert rel_err(ctx.mass_diag, o.diagV) <= 1e-13
    x = rng.uniform(-1, 1, prob.N)
    y = ctx.zeros(prob.N)
    ctx.mass_set_ess(0)
    ctx.mass_mult(0, ctx.to_dev(x), y)
    want = o.mass_mult(0, x, comp=0)
    assert np.all(want[prob.ess[0]] == 0.0)
    assert rel_err(to_host(y), want) <= 1e-13
    ctx.mass_mult(0, ctx.to_dev(x), y, full=True)
    assert rel_err(to_host(y), o.mass_mult(0, x, comp=0, full=True)) <= 1e-13
    xl = rng.uniform(-1, 1, prob.L2V)
    yl = ctx.zeros(prob.L2V)
    ctx.mass_mult(1, ctx.to_dev(xl), yl)
    assert rel_err(to_host(yl), o.mass_mult(1, xl)) <= 1e-13
    ctx.l2_mass_solve_local(ctx.to_dev(xl), yl)
    assert rel_err(to_host(yl), o.l2_solve_local(xl)) <= 1e-12


def test_force_products(pair):
    """F x and F^T v with the same stress data on both sides (ForceIntegrator, laghos_assembly.cpp:43-78)."""
    prob, g, o = pair
    rng = np.random.default_rng(12)
    sJ = rng.uniform(-1, 1, prob.NE * prob.NQ)
    g.ctx.set_stressJinvT(sJ)
    o.stressJinvT[:] = sJ
    xl = rng.uniform(-1, 1, prob.L2V)
    y = g.ctx.zeros(prob.N)
    g.ctx.force_mult(g.ctx.to_dev(xl), y)
    assert rel_err(to_host(y), o.force_mult(xl)) <= 1e-13
    v = rng.uniform(-1, 1, prob.N)
    yl = g.ctx.zeros(prob.L2V)
    g.ctx.force_mult_transpose(g.ctx.to_dev(v), yl)
    assert rel_err(to_host(yl), o.force_mult_transpose(v)) <= 1e-13


def _invert_zone(prob, S, z):
    """Zone z mirrored about its centre: its two vertices trade places, so detJ < 0 at its points."""
    m = np.asarray(prob.h1map).reshape(prob.NE, prob.ND)[z]
    S = S.copy()
    S[m] = S[m[0]] + S[m[-1]] - S[m]
    return S


def _states(prob):
    S = deformed_state(prob)
    neg = S.copy()
    neg[2 * prob.H1V::3] = -0.5                            # e < 0 at some points: clamped at 0 on both sides
    still = S.copy()
    still[prob.H1V:2 * prob.H1V] = 0.0                     # v = 0: no viscosity, the sound speed alone
    return dict(deformed=S, negative_e=neg, v_zero=still, inverted=_invert_zone(prob, S, prob.NE // 2))


@pytest.mark.parametrize("kind", ["deformed", "negative_e", "v_zero", "inverted"])
def test_qupdate_and_dt(pair, kind):
    """UpdateQuadratureData, FA body (laghos_solver.cpp:816-985): stressJinvT and dt_est; an inverted zone gives
    dt_est = 0 exactly on both sides."""
    prob, g, o = pair
    S = _states(prob)[kind]
    o.reset_time_step_estimate()
    o.qdata_is_current = False
    o.update_quadrature_data(S)
    dt_o = o.get_time_step_estimate(S)
    g.reset_time_step_estimate()
    g.reset_quadrature_data()
    g.update_quadrature_data(g.ctx.to_dev(S))
    dt_g = g.get_time_step_estimate(None)
    tol = tol_j(1e-12, prob, prob.initial_state()[0], S)
    assert rel_err(g.ctx.stressJinvT, o.stressJinvT) <= tol
    if kind == "inverted":
        assert dt_o == 0.0 and dt_g == 0.0, (dt_g, dt_o)
    else:
        assert 0.0 < dt_o < np.inf and abs(dt_g - dt_o) <= tol * dt_o, (dt_g, dt_o)


def test_cg_h1(pair):
    """The velocity CG: Jacobi PCG on Mv with the end nodes eliminated; iterations within 1, solution as test_cg_h1."""
    prob, g, o = pair
    b = np.random.default_rng(13).uniform(-0.5, 0.5, prob.N)
    b[prob.ess[0]] = 0.0
    x_o, it_o = o.cg(0, b, comp=0, rel_tol=1e-10, max_iter=2000)
    x = g.ctx.zeros(prob.N)
    g.ctx.mass_set_ess(0)
    it = g.ctx.cg_solve(0, g.ctx.to_dev(b), x, 1e-10, 2000)
    xg = to_host(x)
    assert np.all(np.isfinite(xg))
    if prob.N == len(prob.ess[0]):  # one Q1Q0 zone: every node essential, nothing to solve
        assert it == it_o == 0 and np.all(xg == 0.0)
        return
    assert it_o > 0 and abs(it - it_o) <= 1, (it, it_o)
    assert rel_err(xg, x_o) < 1e-8


def test_density_energies_and_mult(pair):
    """ComputeDensity, the internal and kinetic energies, and one full right-hand side at -cgt 1e-14."""
    from oracle import sedov_error as se
    prob, g, o = pair
    S = deformed_state(prob)
    Sd = g.ctx.to_dev(S)
    rho = g.compute_density(Sd)
    assert rel_err(to_host(rho), se.compute_density(prob, S, np.array(o.rho0DetJ0w))) <= \
        tol_j(1e-12, prob, prob.initial_state()[0], S)
    H1V = prob.H1V
    ie, ke = g.ctx.internal_energy(Sd[2 * H1V:]), g.ctx.kinetic_energy(Sd[H1V:2 * H1V])
    ie_o, ke_o = o.internal_energy(S), o.kinetic_energy(S)
    assert abs(ie - ie_o) <= 1e-13 * abs(ie_o) and abs(ke - ke_o) <= 1e-13 * abs(ke_o)
    dS_o = np.empty_like(S)
    o.qdata_is_current = False
    o.mult(S, dS_o)
    dS = g.ctx.zeros(S.size)
    g.reset_quadrature_data()
    g.mult(Sd, dS)
    got = to_host(dS)
    assert np.all(np.isfinite(got))
    for blk in (slice(0, H1V), slice(H1V, 2 * H1V), slice(2 * H1V, None)):
        assert rel_err(got[blk], dS_o[blk]) <= 1e-10


# ---- whole runs ------------------------------------------------------------------------------------------------------

def _run_parity(prob_fn, steps, ode=4, tol=1e-8, cg_tol=1e-12):
    """_state_parity (test_gpu_configs.py) on a 1D problem: equal RK steps and repeats, |e| to 0.1 tol, state to tol."""
    from laghos_amd.hydro import run
    from oracle.driver import run as orun
    prob = prob_fn()
    r = run(prob, t_final=1e9, max_steps=steps, cg_tol=cg_tol, ode_solver=ode)
    o = orun(prob_fn(), t_final=1e9, max_steps=steps, cg_tol=cg_tol, ode_solver=ode)
    assert (r["steps"], r["repeats"]) == (o["steps"], o["repeats"])
    e_o = float(np.sqrt(np.sum(o["S"][2 * prob.H1V:] ** 2)))
    assert abs(r["e_norm"] - e_o) / e_o < 0.1 * tol
    assert rel_err(r["S"], o["S"]) < tol
    return r, o


@pytest.mark.parametrize("problem", [1, 2], ids=["sedov", "sod"])
@pytest.mark.parametrize("ok,ot", PAIRS, ids=[f"Q{a}Q{b}" for a, b in PAIRS])
def test_runs_vs_oracle(problem, ok, ot):
    """30 RK4 steps of 1D Sedov and Sod on 20 zones at every order pair, -cgt 1e-12."""
    r, o = _run_parity(lambda: problem_1d(20, ok, ot, problem, curved=False), 30)
    assert o["repeats"] > 0  # every one of these runs repeats steps early (dt control, laghos.cpp:748-760)


@pytest.mark.parametrize("ne,ok,ot,steps", [(300, 2, 1, 40), (260, 5, 4, 30)])
def test_runs_above_256_zones(ne, ok, ot, steps):
    """Sod above one workgroup of zones: the multi-block reductions and the strided CG loops inside whole runs."""
    r, o = _run_parity(lambda: problem_1d(ne, ok, ot, 2, curved=False), steps)
    assert o["repeats"] > 0


def test_readme_run5_prefix_repeats():
    """The first 60 RK steps of README run 5 (segment01 -rs 5, Q2Q1, RK4, -cgt 1e-8 as published): the oracle repeats
    6 of them; the GPU must repeat the same ones."""
    from oracle.fem import Problem
    r, o = _run_parity(lambda: Problem(mesh="segment01", rs=5, problem=2), 60, cg_tol=1e-8, tol=1e-6)
    assert o["repeats"] == 6


@pytest.mark.parametrize("ode", [1, 2, 3, 4, 6, 7])
def test_ode_solvers_vs_oracle(ode):
    """-s 1, 2, 3, 4, 6, 7 on 1D Sod (segment01 -rs 3): HIP path vs oracle, and the C++ driver beside both.
    (RK6: Verner's weights of +-176 amplify round-off, as in test_other_rk_integrators_vs_oracle.)"""
    from laghos_amd import host_lib
    from oracle.fem import Problem
    r, o = _run_parity(lambda: Problem(mesh="segment01", rs=3, problem=2), 12, ode=ode, cg_tol=1e-8,
                       tol=1e-8 if ode != 6 else 1e-6)
    sim = host_lib.Sim(["-p", 2, "-m", "data/segment01.mesh", "-rs", 3, "-ms", 12, "-tf", 0.6, "-s", ode, "-q"])
    while sim.step() == 1:
        pass
    e_cpp, steps_cpp = sim.e_norm(), sim.rk_steps
    sim.close()
    assert steps_cpp == r["steps"]
    assert abs(e_cpp - r["e_norm"]) / r["e_norm"] < 1e-9


# ---- -err in 1D ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,ok,ot", [(300, 2, 1), (64, 5, 4)])
def test_density_and_error_1d_vs_oracle(n, ok, ot):
    """ComputeDensity and the error integral in 1D on a deformed state and after a short Sedov run, against
    oracle.sedov_error: 1e-10 (as test_density_and_error_vs_oracle)."""
    from laghos_amd import context as C
    from laghos_amd.hydro import TimeLoop
    from helpers import make_gpu
    from oracle import sedov_error as se
    from oracle.fem import bernstein_table, gauss_legendre, lagrange_tables
    prob = problem_1d(n, ok, ot, problem=1, curved=False, E0=0.25)
    h = make_gpu(prob)
    rdj = np.asarray(h.ctx.rho0DetJ0w)
    t = 0.05
    loop = TimeLoop(h, t_final=t)
    while loop.step():
        pass
    eo = se.err_order(ok, ot)
    pts, wts = gauss_legendre(eo // 2 + 1)
    B, G = lagrange_tables(prob.gll, pts)
    Bl = bernstein_table(ot, pts)
    sol = se.SedovSol(1, 1.4, 1.0, 0.25)
    sol.set_time(t)
    par = C.sedov_setup(1, 1.4, 1.0, 0.25)
    for S in (loop.S, h.ctx.to_dev(deformed_state(prob))):
        S_h = S.cpu().numpy()
        rho = h.compute_density(S)
        rho_o = se.compute_density(prob, S_h, rdj)
        assert rel_err(rho.cpu().numpy(), rho_o) < 1e-10
        err = h.sedov_density_error(S, rho, par, t, [0.0, 0.0, 0.0], wts, B, G, Bl)
        err_o = se.density_error(prob, S_h, rho_o, sol, [0, 0, 0], eo)
        assert err_o > 0 and abs(err - err_o) < 1e-10 * err_o, (err, err_o)
    h.close()


def test_cpp_driver_err_option_1d():
    """`laghos -p 1 -dim 1 -nx 64 -err`: the printed "Density L2 error" against the oracle's value for the oracle's own
    run (states agree to CG tolerance -> 1e-5, as test_cpp_driver_err_option).  The exact solution is SedovSol(dim, E0),
    the reference's convention (see test_sedov_1d_convergence_and_shock)."""
    from oracle import sedov_error as se
    from oracle.driver import run as orun, Hydro
    from oracle.fem import Problem
    tf, n = 0.2, 64
    exe = os.path.join(ROOT, "laghos_amd", "laghos")
    p = subprocess.run([exe, "-p", "1", "-dim", "1", "-nx", str(n), "-rs", "0", "-tf", str(tf), "-err"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stdout + p.stderr
    printed = float(next(l for l in p.stdout.splitlines() if l.startswith("Density L2 error:")).split(":")[1])
    prob = Problem(breaks=[np.linspace(0, 1, n + 1)], order_v=2, order_e=1, problem=1)
    ho = Hydro(prob)
    out = orun(prob, t_final=tf, hydro=ho)
    sol = se.SedovSol(1, 1.4, 1.0, 1.0)
    sol.set_time(tf)
    rho_o = se.compute_density(prob, out["S"], np.array(ho.rho0DetJ0w))
    err_o = se.density_error(prob, out["S"], rho_o, sol, [0, 0, 0], se.err_order(2, 1))
    ho.close()
    assert abs(printed - err_o) < 1e-5 * err_o, (printed, err_o)
