"""The kernels on several ranks in 2D (tests/rank_cases.py: the rank grids; tests/rank_threads.py: one host thread per rank
over the in-process loopback communicator), each against the CPU oracle on the GLOBAL one-rank problem in float64.

A 2D velocity solve is the scalar cg_solve(LGH_SPACE_H1) of lgh_scg.hip, once per component (lgh_k1_form reports -1: no
lockstep solver).  Its several-rank branch - cg_init_k with the fold left pending and cg_init_finish_k, mass_gather_k and
the halo sum every iteration, the all-reduce of (d, A d) looked at by cg_update_k (cg_pending_den), the all-reduce of
(r, z) looked at by the NEXT mass kernel (cg_pending_update), cg_update_finish_k before every host look, owner-weighted
(r, z), the halo-summed initial residual - is reached by no 3D run: every decision is taken by the next kernel of the
sequence from rank-summed values, and one rank deciding differently is a wrong answer or a collective mismatch.

Inputs are seeded GLOBAL vectors sampled onto the ranks.  "Shared copies identical": every rank that holds a node ends
with the same bits for it (rank_cases.gather_nodes asserts it while it builds the global vector).  At most nine contexts
are open at any time: one group of ranks is kept between tests and closed before the next one is built.

Measured on an MI355X, worst over the cases: mass action and force products below 1e-13; scalar CG: the oracle's count on
every rank in every case (16 to 35 iterations), x 1.4e-12 against 1e-8, the true-residual ratio 3.5e-9 to 9.8e-9 against
1.01e-8; L2 CG: the oracle's count (14 to 167), x 4.1e-13; right-hand sides: dx exact, dv 8.7e-14 and de 2.1e-14 against
1e-10, dt 4.2e-14, energies 7.6e-15 against 1e-12.  With cg_solve's owner weights taken out and the essential rows left
unzeroed after the halo sum (every rank still takes the same decisions) 62 of the 72 mass and scalar-CG cases fail.
The module takes 5 s."""
import ctypes

import numpy as np
import pytest

import rank_cases as rc
import shape_cases as sc
from helpers import deformed_state, make_oracle, rel_err, seeded
from rank_threads import Ranks

pytestmark = pytest.mark.gpu

TOL = 1e-13
ALL_GRIDS = list(rc.RANK_GRIDS)
CG_GRIDS = [(2, 1), (2, 2), (3, 1), (3, 3)]
ORDERS_OTHER = [(2, 1), (4, 3)]


# ---- one group of ranks and one oracle at a time ------------------------------------------------------------------------------
_open = {"key": None, "ranks": None, "oracles": {}}


def _close_group():
    if _open["ranks"] is not None:
        _open["ranks"].close()
    _open["key"], _open["ranks"] = None, None


def group(pgrid, mesh, order, problem=1, **kw):
    """(global problem, rank problems, the ranks' operators): kept until another one is asked for"""
    key = (tuple(pgrid), mesh, tuple(order), problem, tuple(sorted(kw.items())))
    glob, probs = rc.problems(pgrid, mesh, order, problem)
    if _open["key"] != key:
        _close_group()
        _open["ranks"] = Ranks(probs, **kw)
        _open["key"] = key
    return glob, probs, _open["ranks"]


def oracle(pgrid, mesh, order, problem=1, **kw):
    key = (tuple(pgrid), mesh, tuple(order), problem, tuple(sorted(kw.items())))
    if key not in _open["oracles"]:
        _open["oracles"][key] = make_oracle(rc.problems(pgrid, mesh, order, problem)[0], **kw)
    return _open["oracles"][key]


@pytest.fixture(scope="module", autouse=True)
def _cleanup():
    yield
    _close_group()
    for o in _open["oracles"].values():
        o.close()
    _open["oracles"].clear()


def k1_form(ctx):
    f = ctypes.c_int(-2)
    from laghos_amd._lib import check
    check(ctx.lib.lgh_k1_form(ctx.h, ctypes.byref(f)))
    return f.value


# ---- mass action with the halo ------------------------------------------------------------------------------------------------
MASS_CASES = [(g, (3, 2)) for g in ALL_GRIDS] + [((2, 2), o) for o in ORDERS_OTHER]


@pytest.mark.parametrize("pgrid,order", MASS_CASES, ids=[f"{rc.grid_id(g)}-{sc.order_id(o)}" for g, o in MASS_CASES])
def test_mass_mult_with_halo(pgrid, order):
    """lgh_mass_mult for comp -1, 0, 1 and lgh_mass_mult_full on the graded mesh: every rank's entries against the oracle's
    global product to 1e-13, essential rows exactly 0.0, shared copies identical"""
    glob, probs, R = group(pgrid, "graded", order)
    o = oracle(pgrid, "graded", order)
    xg = seeded(glob.N, 11)
    for comp, full in ((-1, False), (0, False), (1, False), (1, True)):
        yg_o = o.mass_mult(0, xg, comp=comp, full=full)

        def body(r, g, p):
            ctx = g.ctx
            y = ctx.empty(p.N)
            ctx.mass_set_ess(comp)
            ctx.mass_mult(0, ctx.to_dev(rc.slice_nodes(p, xg)), y, full=full)
            ctx.sync()
            return y.cpu().numpy()
        ys = R.run(body)
        for p, y in zip(probs, ys):
            err = rel_err(y, yg_o[rc.node_map(p)])
            assert err < TOL, (comp, full, p.rank, err)
            if comp >= 0 and not full and len(p.ess[comp]):
                assert np.all(y[p.ess[comp]] == 0.0)
        yg = rc.gather_nodes(probs, ys)
        assert rel_err(yg, yg_o) < TOL
        if full:   # (the full product keeps the essential rows: they are not zero)
            assert np.all(yg[glob.ess[1]] != 0.0)


# ---- force products with the halo ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pgrid", [(2, 2), (3, 1)], ids=rc.grid_id)
def test_force_products_with_halo(pgrid):
    """lgh_force_mult (halo of `dim` components) and lgh_force_mult_transpose on a seeded global stressJinvT sliced per rank:
    1e-13 against the oracle, the adjoint identity over all ranks to 1e-12 with the H1 side weighted by `owner`, shared
    copies identical"""
    order = (3, 2)
    glob, probs, R = group(pgrid, "graded", order)
    o = oracle(pgrid, "graded", order)
    sJ = seeded(glob.NE * glob.NQ * glob.dim ** 2, 6)
    e, w = seeded(glob.L2V, 7), seeded(glob.H1V, 8)
    o.stressJinvT[:] = sJ
    Fe_o, Ftw_o = o.force_mult(e), o.force_mult_transpose(w)

    def body(r, g, p):
        ctx = g.ctx
        ctx.set_stressJinvT(rc.slice_stress(p, sJ))
        Fe, Ftw = ctx.empty(p.H1V), ctx.empty(p.L2V)
        ctx.force_mult(ctx.to_dev(rc.slice_zones(p, e, p.NL)), Fe)
        ctx.force_mult_transpose(ctx.to_dev(rc.slice_nodes(p, w, p.dim)), Ftw)
        ctx.sync()
        return Fe.cpu().numpy(), Ftw.cpu().numpy()
    out = R.run(body)
    lhs = rhs = 0.0
    for p, (Fe, Ftw) in zip(probs, out):
        assert rel_err(Fe, rc.slice_nodes(p, Fe_o, p.dim)) < TOL
        assert rel_err(Ftw, rc.slice_zones(p, Ftw_o, p.NL)) < TOL
        own = np.tile(p.owner, p.dim)
        lhs += float((own * rc.slice_nodes(p, w, p.dim)) @ Fe)      # shared nodes count once
        rhs += float(Ftw @ rc.slice_zones(p, e, p.NL))
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1.0)
    Fe_g = rc.gather_nodes(probs, [x[0] for x in out], glob.dim)
    assert rel_err(Fe_g, Fe_o) < TOL


# ---- the scalar H1 CG over the ranks ------------------------------------------------------------------------------------------
def _h1_solve(R, probs, bg, x0g, comp, tol, cap):
    """lgh_cg_solve(LGH_SPACE_H1) on every rank: ([iterations], [x pieces]); lgh_k1_form must say that no lockstep solver
    exists for this context (2D) - the scalar CG is what ran"""
    def body(r, g, p):
        ctx = g.ctx
        if p.dim == 2:
            assert k1_form(ctx) == -1
        x = ctx.zeros(p.N) if x0g is None else ctx.to_dev(rc.slice_nodes(p, x0g))
        ctx.mass_set_ess(comp)
        it = ctx.cg_solve(0, ctx.to_dev(rc.slice_nodes(p, bg)), x, tol, cap)
        ctx.sync()
        return it, x.cpu().numpy()
    out = R.run(body)
    return [o_[0] for o_ in out], [o_[1] for o_ in out]


def _rhs(glob, comp, seed=12):
    b = seeded(glob.N, seed)
    b[glob.ess[comp]] = 0.0
    return b


H1_CASES = [(g, (3, 2)) for g in CG_GRIDS] + [((2, 2), o) for o in ORDERS_OTHER] + [(rc.GRID_3D, rc.ORDER_3D)]
H1_Q3Q2 = [(g, (3, 2)) for g in CG_GRIDS]
H1_CD = H1_Q3Q2 + [(rc.GRID_3D, rc.ORDER_3D)]
_h1_ids = lambda cases: [f"{rc.grid_id(g)}-{sc.order_id(o)}" for g, o in cases]


@pytest.mark.parametrize("start", ["zero", "guess"])
@pytest.mark.parametrize("comp", [0, 1])
@pytest.mark.parametrize("pgrid,order", H1_CASES, ids=_h1_ids(H1_CASES))
def test_h1_cg_parity(pgrid, order, comp, start):
    """(a) tolerance 1e-10, cap 300, against the oracle's global CG: the same count on every rank and within 1 of the
    oracle's, the solution within 1e-8 (the bounds of test_cg_h1), shared copies identical - from x = 0 and from a seeded
    guess sampled consistently onto the ranks (the halo-summed A x of the initial residual)"""
    glob, probs, R = group(pgrid, "graded", order)
    o = oracle(pgrid, "graded", order)
    bg = _rhs(glob, comp)
    x0g = None
    if start == "guess":
        x0g = seeded(glob.N, 14)
        x0g[glob.ess[comp]] = 0.0
    x_o, it_o = o.cg(0, bg.copy(), x=None if x0g is None else x0g.copy(), comp=comp, rel_tol=1e-10, max_iter=300)
    its, xs = _h1_solve(R, probs, bg, x0g, comp, 1e-10, 300)
    xg = rc.gather_nodes(probs, xs)
    print(f"FIG h1-parity {rc.grid_id(pgrid)} {sc.order_id(order)} comp {comp} {start}: iterations {its} oracle {it_o} x {rel_err(xg, x_o):.2e}")
    assert len(set(its)) == 1, its
    assert 0 < it_o < 300 and abs(its[0] - it_o) <= 1, (its, it_o)
    assert rel_err(xg, x_o) < 1e-8


@pytest.mark.parametrize("comp", [0, 1])
@pytest.mark.parametrize("pgrid,order", H1_Q3Q2, ids=_h1_ids(H1_Q3Q2))
def test_h1_cg_true_residual(pgrid, order, comp):
    """(b) tolerance 1e-8 from x = 0: the TRUE residual r = b - M x of the gathered solution, formed by the oracle in
    float64, satisfies sqrt((r, D^-1 r) / (b, D^-1 b)) <= 1.01e-8, D the oracle's Jacobi diagonal.  The kernels test the
    recurrence residual, which differs from the true one by rounding of order 1e-16 x iterations x cond - about 1e-13 here,
    five orders below the tolerance: the margin of one per cent is far above it.  Fails if any rank stops early, drops a
    shared contribution or weights a shared node twice."""
    glob, probs, R = group(pgrid, "graded", order)
    o = oracle(pgrid, "graded", order)
    bg = _rhs(glob, comp, seed=15)
    its, xs = _h1_solve(R, probs, bg, None, comp, 1e-8, 300)
    xg = rc.gather_nodes(probs, xs)
    r = bg - o.mass_mult(0, xg, comp=comp)
    D = np.array(o.diagV)
    ratio = float(np.sqrt((r @ (r / D)) / (bg @ (bg / D))))
    print(f"FIG h1-true-residual {rc.grid_id(pgrid)} comp {comp}: iterations {its} ratio {ratio:.4e}")
    assert len(set(its)) == 1 and 0 < its[0] < 300, its
    assert ratio <= 1.01e-8


@pytest.mark.parametrize("comp", [0, 1])
@pytest.mark.parametrize("pgrid,order", H1_CD, ids=_h1_ids(H1_CD))
def test_h1_cg_cut_short(pgrid, order, comp):
    """(c) tolerance 1e-14, cap 3: every rank reports 3 iterations, x is the oracle's iterate after three iterations to
    1e-12, shared copies identical"""
    glob, probs, R = group(pgrid, "graded", order)
    o = oracle(pgrid, "graded", order)
    bg = _rhs(glob, comp)
    x_o, it_o = o.cg(0, bg.copy(), comp=comp, rel_tol=1e-14, max_iter=3)
    assert it_o == 3
    its, xs = _h1_solve(R, probs, bg, None, comp, 1e-14, 3)
    xg = rc.gather_nodes(probs, xs)
    assert its == [3] * len(probs), its
    assert rel_err(xg, x_o) < 1e-12


@pytest.mark.parametrize("comp", [0, 1])
@pytest.mark.parametrize("pgrid,order", H1_CD, ids=_h1_ids(H1_CD))
def test_h1_cg_rhs_inside_one_block(pgrid, order, comp):
    """(d) a right-hand side that lives in the interior of the LAST rank's block, zero elsewhere: the other ranks' local
    (r, z) start at zero, so the decision to start at all has to be the collective one.  Asserts as in (a)."""
    glob, probs, R = group(pgrid, "graded", order)
    o = oracle(pgrid, "graded", order)
    last = probs[-1]
    inside = np.ones(last.nn[::-1], dtype=bool)
    for ax in range(last.dim):
        sl = [slice(None)] * last.dim
        for edge in (0, -1):
            sl[ax] = edge
            inside[tuple(sl)] = False
    gi = rc.node_map(last)[inside.reshape(-1)]
    bg = np.zeros(glob.N)
    bg[gi] = seeded(gi.size, 16)
    for p in probs[:-1]:
        assert not np.any(rc.slice_nodes(p, bg))
    x_o, it_o = o.cg(0, bg.copy(), comp=comp, rel_tol=1e-10, max_iter=300)
    its, xs = _h1_solve(R, probs, bg, None, comp, 1e-10, 300)
    xg = rc.gather_nodes(probs, xs)
    assert len(set(its)) == 1, its
    assert 0 < it_o < 300 and abs(its[0] - it_o) <= 1, (its, it_o)
    assert rel_err(xg, x_o) < 1e-8
    assert all(np.any(x) for x in xs)   # (the mass matrix couples the blocks: every rank ends with a part of the solution)


@pytest.mark.parametrize("comp", [0, 1])
@pytest.mark.parametrize("pgrid,order", H1_Q3Q2, ids=_h1_ids(H1_Q3Q2))
def test_h1_cg_zero_rhs(pgrid, order, comp):
    """(e) zero right-hand side on every rank from x = 0 (the energy right-hand side of every Sedov run's first stage is
    such a state): every rank returns 0 iterations and x stays exactly zero"""
    glob, probs, R = group(pgrid, "graded", order)
    its, xs = _h1_solve(R, probs, np.zeros(glob.N), None, comp, 1e-10, 300)
    assert its == [0] * len(probs), its
    for x in xs:
        assert np.all(x.view(np.int64) == 0)


# ---- the L2 CG over the ranks -------------------------------------------------------------------------------------------------
L2_CASES = [(g, o) for g in [(2, 2), (3, 1)] for o in [(2, 1), (3, 2), (4, 3)]]


@pytest.mark.parametrize("pgrid,order", L2_CASES, ids=_h1_ids(L2_CASES))
def test_l2_cg(pgrid, order):
    """lgh_cg_solve(LGH_SPACE_L2): the bounds of test_cg_l2 (count within a tenth of the oracle's, solution 1e-8), the same
    count on all ranks; and the zero right-hand side as in (e).  Graded mesh up to Q3Q2, equal mesh at Q4Q3
    (shape_cases.solve_mesh: the unpreconditioned CG needs thousands of iterations on a graded mesh there)."""
    mesh = sc.solve_mesh(order)
    glob, probs, R = group(pgrid, mesh, order)
    o = oracle(pgrid, mesh, order)
    bg = seeded(glob.L2V, 13)
    x_o, it_o = o.cg(1, bg.copy(), rel_tol=1e-10, max_iter=300)

    def solve(b):
        def body(r, g, p):
            ctx = g.ctx
            x = ctx.zeros(p.L2V)
            it = ctx.cg_solve(1, ctx.to_dev(rc.slice_zones(p, b, p.NL)), x, 1e-10, 300)
            ctx.sync()
            return it, x.cpu().numpy()
        out = R.run(body)
        return [o_[0] for o_ in out], rc.gather_zones(probs, [o_[1] for o_ in out], glob.NL)
    its, xg = solve(bg)
    print(f"FIG l2 {rc.grid_id(pgrid)} {sc.order_id(order)}: iterations {its} oracle {it_o} x {rel_err(xg, x_o):.2e}")
    assert len(set(its)) == 1, its
    assert 0 < it_o < 300 and abs(its[0] - it_o) <= max(1, it_o // 10), (its, it_o)
    assert rel_err(xg, x_o) < 1e-8
    its, xg = solve(np.zeros(glob.L2V))
    assert its == [0] * len(probs), its
    assert np.all(xg.view(np.int64) == 0)


# ---- one right-hand-side evaluation, the time-step estimate, the energies -------------------------------------------------------
RHS_CASES = ([(g, (3, 2), prob) for prob in (1, 0, 7) for g in [(2, 2), (3, 1)]] + [((2, 2), o, 1) for o in ORDERS_OTHER])


@pytest.mark.parametrize("timers", [0, 1], ids=["timers-off", "timers-on"])
@pytest.mark.parametrize("pgrid,order,problem", RHS_CASES, ids=[f"{rc.grid_id(g)}-{sc.order_id(o)}-p{p}" for g, o, p in RHS_CASES])
def test_rhs_on_ranks(pgrid, order, problem, timers):
    """HydroOperator(prob_r, comm=...) on helpers.deformed_state of the global problem, both CGs at 1e-14: dS/dt against the
    oracle's mult with the bounds of test_hydro_mult (dx 1e-13, dv and de 1e-10), the time-step estimate to 1e-12 and
    identical on all ranks, internal and kinetic energy to 1e-12 (test_energies) with the same bits on every rank.
    Problem 1: viscosity; problem 0: lgh_tg_source_2d on rank-local zones, no viscosity; problem 7: vorticity, and the
    gravity source through the halo-summed MultFull.  Region timers change the sequencing of lgh_solve_velocity and make
    the energy solve sequential: both are run.  Mesh by shape_cases.solve_mesh, as for the L2 CG."""
    mesh = sc.solve_mesh(order)
    kw = dict(cg_tol=sc.CG_TOL, cg_max_iter=sc.CG_CAP)
    glob, probs, R = group(pgrid, mesh, order, problem, **kw)
    o = oracle(pgrid, mesh, order, problem, **kw)
    S = deformed_state(glob, seed=21)
    dS_o = np.empty_like(S)
    o.reset_time_step_estimate()
    o.qdata_is_current = False
    dt_o = o.get_time_step_estimate(S)
    o.reset_timers()
    o.mult(S, dS_o)
    t_o = o.timers()
    assert t_o["L2iter"] < sc.CG_CAP and t_o["H1iter"] < sc.CG_CAP
    ie_o, ke_o = o.internal_energy(S), o.kinetic_energy(S)

    def body(r, g, p):
        import torch
        ctx = g.ctx
        if p.dim == 2:
            assert k1_form(ctx) == -1
        ctx.enable_timers(bool(timers))
        ctx.reset_timers()
        Sd = ctx.to_dev(rc.slice_state(p, S))
        dS = ctx.zeros(Sd.numel())
        torch.cuda.current_stream(ctx.device).synchronize()
        g.reset_time_step_estimate()
        g.reset_quadrature_data()
        dt = g.get_time_step_estimate(Sd)
        g.mult(Sd, dS)
        ctx.sync()
        ie = ctx.internal_energy(Sd[2 * p.H1V:])
        ke = ctx.kinetic_energy(Sd[p.H1V:2 * p.H1V])
        return dict(dS=dS.cpu().numpy(), dt=dt, ie=ie, ke=ke, t=ctx.timers())
    out = R.run(body)
    H1V = glob.H1V
    dx = rc.gather_nodes(probs, [x["dS"][:p.H1V] for p, x in zip(probs, out)], glob.dim)
    dv = rc.gather_nodes(probs, [x["dS"][p.H1V:2 * p.H1V] for p, x in zip(probs, out)], glob.dim)
    de = rc.gather_zones(probs, [x["dS"][2 * p.H1V:] for p, x in zip(probs, out)], glob.NL)
    fig = (rel_err(dx, dS_o[:H1V]), rel_err(dv, dS_o[H1V:2 * H1V]), rel_err(de, dS_o[2 * H1V:]))
    print(f"FIG rhs {rc.grid_id(pgrid)} {sc.order_id(order)} p{problem} timers {timers}: dx {fig[0]:.2e} dv {fig[1]:.2e} de {fig[2]:.2e} "
          f"dt {abs(out[0]['dt'] - dt_o) / dt_o:.2e} ie {abs(out[0]['ie'] - ie_o) / abs(ie_o):.2e} ke {abs(out[0]['ke'] - ke_o) / abs(ke_o):.2e}")
    assert np.all(np.isfinite(dx)) and np.all(np.isfinite(dv)) and np.all(np.isfinite(de))
    if timers:
        assert all(x["t"]["H1iter"] < sc.CG_CAP and x["t"]["L2iter"] < sc.CG_CAP for x in out)
        assert len({(x["t"]["H1iter"], x["t"]["L2iter"]) for x in out}) == 1
    assert fig[0] < TOL
    assert fig[1] < 1e-10
    assert fig[2] < 1e-10
    assert len({x["dt"] for x in out}) == 1 and abs(out[0]["dt"] - dt_o) <= 1e-12 * dt_o
    assert len({(x["ie"], x["ke"]) for x in out}) == 1, [(x["ie"], x["ke"]) for x in out]
    assert abs(out[0]["ie"] - ie_o) <= 1e-12 * abs(ie_o)
    assert abs(out[0]["ke"] - ke_o) <= 1e-12 * abs(ke_o)


def test_no_lockstep_energy_solve_on_2d_ranks(monkeypatch):
    """2D has no lockstep velocity solve, hence no energy solve in lockstep with it, with one communicator (LGH_COMM2=0) or
    two: lgh_energy_lockstep_stats reports zeros and out[3] == 0 after right-hand sides on 2 x 2 ranks"""
    from laghos_amd._lib import check
    for comm2 in ("0", "1"):
        monkeypatch.setenv("LGH_COMM2", comm2)
        _close_group()   # (the switch is read when the communicator is made)
        glob, probs, R = group((2, 2), "graded", (3, 2), 1)
        S = deformed_state(glob, seed=21)

        def body(r, g, p):
            ctx = g.ctx
            ctx.enable_timers(False)
            Sd = ctx.to_dev(rc.slice_state(p, S))
            dS = ctx.zeros(Sd.numel())
            for _ in range(2):
                g.reset_quadrature_data()
                g.mult(Sd, dS)
            ctx.sync()
            ls = (ctypes.c_long * 4)()
            check(ctx.lib.lgh_energy_lockstep_stats(ctx.h, ls))
            return list(ls)
        out = R.run(body)
        assert out == [[0, 0, 0, 0]] * 4, out
        _close_group()
