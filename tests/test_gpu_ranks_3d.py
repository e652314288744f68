"""The kernels on several ranks in 3D (tests/rank_cases.py: the 3D table; tests/rank_threads.py: one host thread per rank
over the in-process loopback communicator), each against the CPU oracle on the GLOBAL one-rank problem in float64.

In 3D every velocity solve on several ranks is the lockstep solver of lgh_vcg.hip in its several-rank mode: K2 reads
halo-summed values at shared nodes and weights (r, z) by `owner`; (d, A d) rides on the halo messages on all-pairs partitions
and goes through the all-reduce elsewhere; (r, z) crosses the ranks as exact accumulator words or as ticketed doubles; K2
fills the send buffers itself; the node lists are translated into the library's own order (HaloNodeAlias); the energy CG
can run in lockstep with its sums on the velocity iteration's messages.  vcg_mode_collective decides all of it at the first
solve, and every rank has to decide alike.  The whole runs that reach this code compare scalars of a several-rank run with
the one-rank GPU run on equal meshes; here every entry of every result is held to the oracle, on graded meshes (every zone
its own mass factor and Jac0inv) up to Q3Q2 and on the equal mesh at Q4Q3 and Q5Q4 (shape_cases.solve_mesh).

Inputs are seeded GLOBAL vectors and states sliced per rank.  "Shared copies identical": every rank that holds a node ends
with the same bits for it (rank_cases.gather_nodes asserts it while it builds the global vector).  At most nine contexts
are open at any time: one group of ranks is kept between tests and closed before the next one is built; the environment
switches are set before a group is built, since a context reads them once.  Every lockstep test asserts the form of K1
(plane, column, slab, kron) the case means.

Cases that are left out: problem 3 - on the breaks of rank_cases (a box of 1 x 1.25 x 1.5) its interfaces x = 1, y = 1.5 and
z = 1.5 lie on or outside the boundary, so no material crosses a rank boundary.  Problem 7 runs on 2 x 2 x 1 ranks: the
oracle's set-up (rho0 and e0 by y, gravity along -y, vorticity) is the same in 3D; on these breaks the whole box is the
heavy fluid, what the case adds is the acceleration source through the halo-summed MultFull.  The device reports the
iterations of the three component solves as one total, so counts are compared as totals (within `dim` of the oracle's).

Measured on an MI355X, worst over the cases: mass action 5.8e-15, force products 5.9e-16, adjoint identity 6.7e-15.
Right-hand sides: dx exact; dv 1.3e-14 (Q2Q1), 5.4e-14 (Q3Q2, all forms, grids and switch settings), 4.2e-13 (Q4Q3), 6.6e-13
(Q5Q4) against 1e-10; de 1.4e-14, 1.7e-13, 4.1e-13 against 1e-10 and 6.8e-13 (Q5Q4) against 1e-8; dt 1.4e-14, 7.2e-14, 3.6e-13
and 6.5e-13 against 1e-12; energies 1.7e-14 against 1e-12.  The velocity solves take the oracle's total on every rank in every
case (110 to 147 iterations), the energy solve 47 to 693 against the oracle's 47 to 696 (at most 12 apart).  Velocity solve
alone: cut short 9 iterations on every rank, dv 4.1e-14 against 1e-12; the blast 80 (oracle 27 + 27 + 26) and 68 (22 + 23 + 23)
iterations on every rank, dv 7.1e-11 against 1e-8; second solve 5.2e-14.  Switch settings against the default: de identical
in every setting, dv identical with HALO_FUSED_PACK=0 and COMM2=0 and, on 3 x 1 x 1, with every setting but SLAB_MERGE=0; else at
most 8.5e-16 apart.  The energy solve in lockstep: one solve per rank, 40 (2 x 1 x 1) and 43 (2 x 2 x 2) of its iterations
inside the velocity solve.
dt at Q4Q3 and Q5Q4 on 2 x 2 x 2 ranks comes within a factor of 10 of its bar.  That is the reference's own error and no
matter of ranks: the oracle's mesh volume of the 10 x 6 x 4 box, summed through the gradient tables of degree 4 and 5, is off
the exact 1.875 by -6.6e-13 and 1.0e-12, the device's by less than 1e-15; h0 takes a third of that, and dt, dv and de carry it
(one rank against the oracle on the same mesh: dt 6.5e-13, dv 6.6e-13 - the figures of eight ranks; on 15 x 2 x 2 zones the
volumes agree to 1.2e-14 and dt to 2.0e-14).
With the owner weight of K2's (r, z) set to 1.0 (every rank still takes the same decisions) 65 of the 83 cases fail: all of
(b) to (f) but the four zero right-hand sides, which never reach K2; the mass and force cases do not run K2.
The module takes 19 s."""
import ctypes

import numpy as np
import pytest

import rank_cases as rc
import shape_cases as sc
from helpers import deformed_state, make_oracle, rel_err, seeded
from rank_threads import Ranks

pytestmark = pytest.mark.gpu

TOL = 1e-13
GRIDS = list(rc.RANK_GRIDS_3D)
SWITCHES = ("LGH_VCG_VARIANT", "LGH_HALO_PIGGYBACK", "LGH_HALO_FUSED_PACK", "LGH_RZ_LIMBS", "LGH_SLAB_DEFER", "LGH_SLAB_MERGE",
            "LGH_COMM2", "LGH_ENERGY_LOCKSTEP", "LGH_ORDER_MULTI")
FORM_ENV = {"column": {"LGH_VCG_VARIANT": "0"}, "slab": {"LGH_VCG_VARIANT": "4"}, "kron": {"LGH_VCG_VARIANT": "5"}}
CG = dict(cg_tol=sc.CG_TOL, cg_max_iter=sc.CG_CAP)


def default_form(order):
    """the default dispatch of K1 (lgh_vcg_k1.hip::vcg_resolve_k1) below the slab threshold: the Kronecker form from Q4Q3"""
    return "kron" if order[0] >= 4 else "plane"


def _env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return env


def _env_id(env):
    return ",".join(f"{k[4:]}={v}" for k, v in env.items()) or "default"


# ---- one group of ranks and one oracle at a time ------------------------------------------------------------------------------
_open = {"key": None, "ranks": None, "oracles": {}}


def _close_group():
    if _open["ranks"] is not None:
        _open["ranks"].close()
    _open["key"], _open["ranks"] = None, None


def group(pgrid, mesh, order, problem=1, env=None, perm_seed=None, **kw):
    """(global problem, rank problems, the ranks' operators): kept until another one is asked for.  env: the switches the
    caller has SET (part of the key: a context reads them once).  perm_seed: every rank's block under
    rank_cases.permuted_rank with its own seed; the rank problems returned are those wrappers."""
    key = (tuple(pgrid), mesh, tuple(order), problem, tuple(sorted((env or {}).items())), perm_seed, tuple(sorted(kw.items())))
    glob, probs = rc.problems(pgrid, mesh, order, problem)
    if perm_seed is not None:
        probs = [rc.permuted_rank(p, seed=perm_seed + p.rank) for p in probs]
    if _open["key"] != key:
        _close_group()
        _open["ranks"] = Ranks(probs, **kw)
        _open["key"] = key
    return glob, _open["ranks"].probs, _open["ranks"]


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


def lockstep_stats(ctx):
    from laghos_amd._lib import check
    ls = (ctypes.c_long * 4)()
    check(ctx.lib.lgh_energy_lockstep_stats(ctx.h, ls))
    return dict(solves=ls[0], inside=ls[1], after=ls[2], ready=ls[3])


# ---- (a) mass action and force products with the halo, three components -----------------------------------------------------
HALO_CASES = [(g, (3, 2)) for g in GRIDS] + [((2, 2, 2), o) for o in [(2, 1), (4, 3)]]
_case_ids = lambda cases: [f"{rc.grid_id(g)}-{sc.order_id(o)}" for g, o in cases]


@pytest.mark.parametrize("pgrid,order", HALO_CASES, ids=_case_ids(HALO_CASES))
def test_mass_mult_with_halo(pgrid, order, monkeypatch):
    """lgh_mass_mult for comp -1, 0, 1, 2 and lgh_mass_mult_full on the graded mesh: every rank's entries against the oracle's
    global product to 1e-13, essential rows exactly 0.0, shared copies identical"""
    _env(monkeypatch, {})
    glob, probs, R = group(pgrid, "graded", order)
    o = oracle(pgrid, "graded", order)
    xg = seeded(glob.N, 11)
    worst = 0.0
    for comp, full in ((-1, False), (0, False), (1, False), (2, False), (2, True)):
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
            worst = max(worst, err)
            assert err < TOL, (comp, full, p.rank, err)
            if comp >= 0 and not full and len(p.ess[comp]):
                assert np.all(y[p.ess[comp]] == 0.0)
        yg = rc.gather_nodes(probs, ys)
        assert rel_err(yg, yg_o) < TOL
        if full:   # (the full product keeps the essential rows: they are not zero)
            assert np.all(yg[glob.ess[2]] != 0.0)
    print(f"FIG mass {rc.grid_id(pgrid)} {sc.order_id(order)}: {worst:.2e}")


@pytest.mark.parametrize("pgrid,order", HALO_CASES, ids=_case_ids(HALO_CASES))
def test_force_products_with_halo(pgrid, order, monkeypatch):
    """lgh_force_mult (halo of three components) and lgh_force_mult_transpose on a seeded global stressJinvT sliced per
    rank: 1e-13 against the oracle, the adjoint identity over all ranks to 1e-12 with the H1 side weighted by `owner`,
    shared copies identical"""
    _env(monkeypatch, {})
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
    worst = 0.0
    for p, (Fe, Ftw) in zip(probs, out):
        errs = rel_err(Fe, rc.slice_nodes(p, Fe_o, p.dim)), rel_err(Ftw, rc.slice_zones(p, Ftw_o, p.NL))
        worst = max(worst, *errs)
        assert errs[0] < TOL and errs[1] < TOL, (p.rank, errs)
        own = np.tile(p.owner, p.dim)
        lhs += float((own * rc.slice_nodes(p, w, p.dim)) @ Fe)      # shared nodes count once
        rhs += float(Ftw @ rc.slice_zones(p, e, p.NL))
    adj = abs(lhs - rhs) / max(abs(lhs), abs(rhs), 1.0)
    print(f"FIG force {rc.grid_id(pgrid)} {sc.order_id(order)}: {worst:.2e} adjoint {adj:.2e}")
    assert adj <= 1e-12
    Fe_g = rc.gather_nodes(probs, [x[0] for x in out], glob.dim)
    assert rel_err(Fe_g, Fe_o) < TOL


# ---- (b) one right-hand side on ranks, per form of K1 -------------------------------------------------------------------------
_oracle_rhs = {}


def oracle_rhs(pgrid, order, problem=1, seed=21):
    """The oracle's right-hand side, time-step estimate and energies on helpers.deformed_state of the global problem: computed
    once per (grid, order, problem, seed), shared by the forms and switch settings, never modified.  Its own iteration
    counts stay below the cap on this state: a condition of the input, asserted here."""
    key = (tuple(pgrid), tuple(order), problem, seed)
    if key not in _oracle_rhs:
        mesh = sc.solve_mesh(order)
        glob = rc.problems(pgrid, mesh, order, problem)[0]
        o = oracle(pgrid, mesh, order, problem, **CG)
        S = deformed_state(glob, seed=seed)
        dS = np.empty_like(S)
        o.reset_time_step_estimate()
        o.qdata_is_current = False
        dt = o.get_time_step_estimate(S)
        o.reset_timers()
        o.mult(S, dS)
        t = o.timers()
        assert t["L2iter"] < sc.CG_CAP and t["H1iter"] < sc.CG_CAP, t
        ref = dict(S=S, dS=dS, dt=dt, ie=o.internal_energy(S), ke=o.kinetic_energy(S), H1iter=t["H1iter"], L2iter=t["L2iter"])
        for k in ("S", "dS"):
            ref[k].setflags(write=False)
        _oracle_rhs[key] = ref
    return _oracle_rhs[key]


def run_rhs(R, probs, S, timers, form, extra=None):
    """HydroOperator.mult on every rank's piece of the global state(s) S (a list: one call each on the same contexts; the
    last one is returned), with the time-step estimate and the energies.  Rank problems under rank_cases.permuted_rank take
    their piece in their own numbering and hand the result back in the generator's."""
    states = S if isinstance(S, list) else [S]

    def body(r, g, p):
        import torch
        ctx = g.ctx
        assert ctx.k1_form() == form, (ctx.k1_form(), form)
        base = getattr(p, "base", p)
        ctx.enable_timers(bool(timers))
        for Sg in states:
            piece = rc.slice_state(base, Sg)
            Sd = ctx.to_dev(p.state(piece) if base is not p else piece)
            dS = ctx.zeros(Sd.numel())
            torch.cuda.current_stream(ctx.device).synchronize()
            ctx.reset_timers()
            g.reset_time_step_estimate()
            g.reset_quadrature_data()
            dt = g.get_time_step_estimate(Sd)
            g.mult(Sd, dS)
            ctx.sync()
        ie = ctx.internal_energy(Sd[2 * p.H1V:])
        ke = ctx.kinetic_energy(Sd[p.H1V:2 * p.H1V])
        dS = dS.cpu().numpy()
        H1V = base.H1V
        if base is not p:
            dS = np.concatenate([rc.unpermute_nodes(p, dS[:H1V], p.dim), rc.unpermute_nodes(p, dS[H1V:2 * H1V], p.dim),
                                 rc.unpermute_zones(p, dS[2 * H1V:], p.NL)])
        return dict(dS=dS, dt=dt, ie=ie, ke=ke, t=ctx.timers(), ls=lockstep_stats(ctx), extra=extra(ctx) if extra else None)
    return R.run(body)


def check_rhs(tag, glob, probs, out, ref, order, timers):
    """the bars of test_rhs_on_ranks (2D) and test_gpu_shapes_solve.py::test_rhs: dx/dt 1e-13, dv/dt and de/dt 1e-10 (de/dt
    1e-8 at Q5Q4), dt_est to 1e-12 and identical on all ranks, the energies to 1e-12 with the same bits on every rank; with
    timers on, the same iteration counts on all ranks, below the cap.  Returns the gathered (dv, de)."""
    base = [getattr(p, "base", p) for p in probs]
    H1V, dS_o = glob.H1V, ref["dS"]
    dx = rc.gather_nodes(base, [x["dS"][:p.H1V] for p, x in zip(base, out)], glob.dim)
    dv = rc.gather_nodes(base, [x["dS"][p.H1V:2 * p.H1V] for p, x in zip(base, out)], glob.dim)
    de = rc.gather_zones(base, [x["dS"][2 * p.H1V:] for p, x in zip(base, out)], glob.NL)
    fig = (rel_err(dx, dS_o[:H1V]), rel_err(dv, dS_o[H1V:2 * H1V]), rel_err(de, dS_o[2 * H1V:]))
    its = sorted({(x["t"]["H1iter"], x["t"]["L2iter"]) for x in out})
    print(f"FIG rhs {tag} timers {timers}: dx {fig[0]:.2e} dv {fig[1]:.2e} de {fig[2]:.2e} dt {abs(out[0]['dt'] - ref['dt']) / ref['dt']:.2e} "
          f"ie {abs(out[0]['ie'] - ref['ie']) / abs(ref['ie']):.2e} ke {abs(out[0]['ke'] - ref['ke']) / abs(ref['ke']):.2e} "
          f"iterations (H1, L2) {its} oracle {(ref['H1iter'], ref['L2iter'])}")
    assert np.all(np.isfinite(dx)) and np.all(np.isfinite(dv)) and np.all(np.isfinite(de))
    if timers:
        assert len(its) == 1, its
        assert 0 < its[0][0] < sc.CG_CAP and 0 < its[0][1] < sc.CG_CAP, its
    assert fig[0] < TOL
    assert fig[1] < 1e-10
    assert fig[2] < (1e-8 if tuple(order) == (5, 4) else 1e-10)
    assert len({x["dt"] for x in out}) == 1 and abs(out[0]["dt"] - ref["dt"]) <= 1e-12 * ref["dt"]
    assert len({(x["ie"], x["ke"]) for x in out}) == 1, [(x["ie"], x["ke"]) for x in out]
    assert abs(out[0]["ie"] - ref["ie"]) <= 1e-12 * abs(ref["ie"])
    assert abs(out[0]["ke"] - ref["ke"]) <= 1e-12 * abs(ref["ke"])
    return dv, de


# (rank grid, order, problem, form of K1)
RHS_CASES = ([(g, (3, 2), 1, "plane") for g in GRIDS]
             + [(g, (3, 2), 1, f) for g in [(2, 2, 2), (3, 1, 1)] for f in ("column", "slab", "kron")]
             + [((2, 2, 2), (2, 1), 1, "plane")]
             + [(g, o, 1, "kron") for o in [(4, 3), (5, 4)] for g in [(2, 2, 2), (3, 1, 1)]]
             + [((2, 2, 1), (3, 2), 7, "plane")])


def _rhs_id(c):
    return f"{rc.grid_id(c[0])}-{sc.order_id(c[1])}-p{c[2]}-{c[3]}"


@pytest.mark.parametrize("timers", [0, 1], ids=["timers-off", "timers-on"])
@pytest.mark.parametrize("pgrid,order,problem,form", RHS_CASES, ids=[_rhs_id(c) for c in RHS_CASES])
def test_rhs_on_ranks(pgrid, order, problem, form, timers, monkeypatch):
    """HydroOperator(prob_r, comm=...).mult on helpers.deformed_state of the global problem, both CGs at 1e-14 with the cap
    of 4000: check_rhs against the oracle.  Q3Q2 on all five grids in the default dispatch (plane) and with every other form of
    K1 forced on 2 x 2 x 2 (all-pairs) and 3 x 1 x 1 (not all-pairs); Q2Q1; Q4Q3 and Q5Q4 in their default Kronecker form on
    the equal mesh; problem 7 on 2 x 2 x 1 ranks (gravity through the halo-summed MultFull, vorticity).  Region timers change
    the sequencing of lgh_solve_velocity and make the energy solve sequential: both are run."""
    env = _env(monkeypatch, {} if form == default_form(order) else FORM_ENV[form])
    ref = oracle_rhs(pgrid, order, problem)
    glob, probs, R = group(pgrid, sc.solve_mesh(order), order, problem, env=env, **CG)
    out = run_rhs(R, probs, ref["S"], timers, form)
    check_rhs(_rhs_id((pgrid, order, problem, form)), glob, probs, out, ref, order, timers)


# ---- (c) the velocity solve alone, at its edges --------------------------------------------------------------------------------
VCG_CASES = [(g, f) for g in [(2, 2, 2), (3, 1, 1)] for f in ("plane", "slab")]
_vcg_ids = [f"{rc.grid_id(g)}-{f}" for g, f in VCG_CASES]


def solve_velocity_on_ranks(R, probs, states, form, tol, cap):
    """g.update_quadrature_data and ctx.solve_velocity on every rank's piece of each global state in turn, on the same
    contexts: per state ([iterations], [dv pieces], [rhs_h1 pieces])"""
    def body(r, g, p):
        ctx = g.ctx
        assert ctx.k1_form() == form, (ctx.k1_form(), form)
        ctx.enable_timers(False)
        res = []
        for Sg in states:
            Sd = ctx.to_dev(rc.slice_state(p, Sg))
            dS = ctx.zeros(Sd.numel())
            g.reset_quadrature_data()
            g.update_quadrature_data(Sd)
            it = ctx.solve_velocity(Sd, dS, None, g.rhs, g.work, tol, cap)
            ctx.sync()
            res.append((it, dS[p.H1V:2 * p.H1V].cpu().numpy(), g.rhs.cpu().numpy()))
        return res
    out = R.run(body)
    return [([o_[k][0] for o_ in out], [o_[k][1] for o_ in out], [o_[k][2] for o_ in out]) for k in range(len(states))]


def oracle_velocity(o, glob, S):
    """(dv, total iterations, -F.1) of the oracle's SolveVelocity at the oracle's own tolerance and cap"""
    dS = np.zeros_like(S)
    o.qdata_is_current = False
    o.reset_timers()
    o.solve_velocity(S, dS)
    rhs = -o.force_mult(np.ones(glob.L2V))
    return dS[glob.H1V:2 * glob.H1V].copy(), o.timers()["H1iter"], rhs


def _vcg_group(pgrid, form, monkeypatch, fresh=False):
    env = _env(monkeypatch, {} if form == "plane" else FORM_ENV[form])
    if fresh:
        _close_group()
    return group(pgrid, "graded", (3, 2), 1, env=env)


@pytest.mark.parametrize("pgrid,form", VCG_CASES, ids=_vcg_ids)
def test_velocity_solve_cut_short(pgrid, form, monkeypatch):
    """tolerance 1e-14, cap 3: every rank reports dim x 3 iterations, dv is the oracle's iterate after three iterations to
    1e-12, shared copies identical"""
    glob, probs, R = _vcg_group(pgrid, form, monkeypatch)
    S = deformed_state(glob, seed=21)
    dv_o, it_o, _ = oracle_velocity(oracle(pgrid, "graded", (3, 2), cg_tol=1e-14, cg_max_iter=3), glob, S)
    assert it_o == 3 * glob.dim
    (its, dvs, _), = solve_velocity_on_ranks(R, probs, [S], form, 1e-14, 3)
    dv = rc.gather_nodes(probs, dvs, glob.dim)
    print(f"FIG vcg-cut-short {rc.grid_id(pgrid)} {form}: iterations {its} dv {rel_err(dv, dv_o):.2e}")
    assert its == [3 * glob.dim] * len(probs), its
    assert rel_err(dv, dv_o) < 1e-12


def blast_state(glob, probs):
    """v = 0 and e = 0 everywhere but in the zones of the LAST rank's block that touch no node another rank holds, where the
    energy dofs are positive"""
    last = probs[-1]
    shared = np.zeros(last.N, dtype=bool)
    for l in last.neighbors()[1]:
        shared[l] = True
    inner = ~np.any(shared[np.asarray(last.h1map)], axis=1)
    assert 0 < inner.sum() < last.NE
    S = glob.initial_state()[0].copy()
    S[glob.H1V:] = 0.0
    e = S[2 * glob.H1V:].reshape(glob.NE, glob.NL)
    e[rc.zone_map(last)[inner]] = 1.0 + seeded((int(inner.sum()), glob.NL), 17)
    return S


@pytest.mark.parametrize("pgrid,form", VCG_CASES, ids=_vcg_ids)
def test_velocity_solve_blast_inside_one_block(pgrid, form, monkeypatch):
    """A pressure that lives strictly inside the LAST rank's block: the oracle's right-hand side is exactly zero at every node
    of every other rank (asserted), so their local (r, z) start at zero and the decision to start at all has to be the
    collective one; the three components finish at different iterations (the oracle's per-component counts, asserted), and
    components that are done send zeros.  Tolerance 1e-10, cap 300: the same count on all ranks, the total within `dim` of
    the oracle's, dv within 1e-8 (the bounds of test_h1_cg_parity), every rank ends with a non-zero part of dv."""
    glob, probs, R = _vcg_group(pgrid, form, monkeypatch)
    o = oracle(pgrid, "graded", (3, 2), cg_tol=1e-10, cg_max_iter=300)
    S = blast_state(glob, probs)
    dv_o, it_o, rhs_o = oracle_velocity(o, glob, S)
    assert np.any(rhs_o)
    for p in probs[:-1]:
        assert not np.any(rc.slice_nodes(p, rhs_o, glob.dim))
    per_comp = []
    for c in range(glob.dim):
        b = rhs_o[c * glob.N:(c + 1) * glob.N].copy()
        b[glob.ess[c]] = 0.0
        per_comp.append(o.cg(0, b, comp=c, rel_tol=1e-10, max_iter=300)[1])
    assert sum(per_comp) == it_o and all(0 < k < 300 for k in per_comp) and len(set(per_comp)) > 1, (per_comp, it_o)
    (its, dvs, _), = solve_velocity_on_ranks(R, probs, [S], form, 1e-10, 300)
    dv = rc.gather_nodes(probs, dvs, glob.dim)
    print(f"FIG vcg-blast {rc.grid_id(pgrid)} {form}: iterations {its} oracle {it_o} {per_comp} dv {rel_err(dv, dv_o):.2e}")
    assert len(set(its)) == 1, its
    assert abs(its[0] - it_o) <= glob.dim, (its, it_o)
    assert rel_err(dv, dv_o) < 1e-8
    assert all(np.any(x) for x in dvs)   # (the mass matrix couples the blocks)


@pytest.mark.parametrize("pgrid,form", VCG_CASES, ids=_vcg_ids)
def test_velocity_solve_nothing_to_do(pgrid, form, monkeypatch):
    """v = 0 and e = 0 everywhere: every rank returns 0 iterations, dv is exactly +0.0 in every entry, rhs_h1 is 0 at the
    essential rows (and everywhere else)"""
    glob, probs, R = _vcg_group(pgrid, form, monkeypatch)
    S = glob.initial_state()[0].copy()
    S[glob.H1V:] = 0.0
    (its, dvs, rhss), = solve_velocity_on_ranks(R, probs, [S], form, 1e-10, 300)
    assert its == [0] * len(probs), its
    for p, dv, rhs in zip(probs, dvs, rhss):
        assert np.all(dv.view(np.int64) == 0)
        for c in range(p.dim):
            assert np.all(rhs[c * p.N + np.asarray(p.ess[c], dtype=np.int64)] == 0.0)
        assert np.all(rhs == 0.0)


@pytest.mark.parametrize("pgrid,form", VCG_CASES, ids=_vcg_ids)
def test_velocity_solve_second_solve_on_the_same_context(pgrid, form, monkeypatch):
    """Two solves on contexts that have not solved before, on two different states at 1e-14 with the cap of 4000: the mode is
    decided once, at the first (vcg_mode_collective: rz_words_all, ls_all); the second is held to the same bars as the first -
    the same count below the cap on all ranks, the total within `dim` of the oracle's, dv to the 1e-10 of check_rhs"""
    glob, probs, R = _vcg_group(pgrid, form, monkeypatch, fresh=True)
    o = oracle(pgrid, "graded", (3, 2), **CG)
    states = [deformed_state(glob, seed=21), deformed_state(glob, seed=22)]
    res = solve_velocity_on_ranks(R, probs, states, form, sc.CG_TOL, sc.CG_CAP)
    for k, (S, (its, dvs, _)) in enumerate(zip(states, res)):
        dv_o, it_o, _ = oracle_velocity(o, glob, S)
        dv = rc.gather_nodes(probs, dvs, glob.dim)
        print(f"FIG vcg-second {rc.grid_id(pgrid)} {form} solve {k}: iterations {its} oracle {it_o} dv {rel_err(dv, dv_o):.2e}")
        assert len(set(its)) == 1 and 0 < its[0] < sc.CG_CAP and 0 < it_o < sc.CG_CAP, (its, it_o)
        assert abs(its[0] - it_o) <= glob.dim, (its, it_o)
        assert rel_err(dv, dv_o) < 1e-10


# ---- (d) the transport switches on ranks ------------------------------------------------------------------------------------------
SETTINGS = ["LGH_HALO_PIGGYBACK", "LGH_HALO_FUSED_PACK", "LGH_RZ_LIMBS", "LGH_SLAB_DEFER", "LGH_SLAB_MERGE", "LGH_COMM2"]
_default_slab = {}


def default_slab_rhs(pgrid, timers, monkeypatch):
    """(dv, de) of the slab form with every transport switch at its default: once per (grid, timers)"""
    if (pgrid, timers) not in _default_slab:
        env = _env(monkeypatch, FORM_ENV["slab"])
        ref = oracle_rhs(pgrid, (3, 2))
        glob, probs, R = group(pgrid, "graded", (3, 2), 1, env=env, **CG)
        out = run_rhs(R, probs, ref["S"], timers, "slab")
        _default_slab[(pgrid, timers)] = check_rhs(f"{rc.grid_id(pgrid)} slab default", glob, probs, out, ref, (3, 2), timers)
    return _default_slab[(pgrid, timers)]


@pytest.mark.parametrize("switch", SETTINGS, ids=[s[4:] + "=0" for s in SETTINGS])
@pytest.mark.parametrize("pgrid", [(2, 2, 2), (3, 1, 1)], ids=rc.grid_id)
def test_transport_switches(pgrid, switch, monkeypatch):
    """The slab form with one transport switch off - the sums beside the halo messages instead of on them, the send buffers
    packed by a kernel of their own, ticketed (r, z) instead of accumulator words, the fold of (d, A d) in K1, the unmerged
    E-vector, no second channel: check_rhs against the oracle, timers off and on.  dv/dt and de/dt are also compared with the
    default setting's and the difference is printed (both are within one bar of the oracle); the settings sum in different
    orders, so bit equality is not claimed."""
    ref = oracle_rhs(pgrid, (3, 2))
    for timers in (0, 1):
        dv0, de0 = default_slab_rhs(pgrid, timers, monkeypatch)
        env = _env(monkeypatch, dict(FORM_ENV["slab"], **{switch: "0"}))
        glob, probs, R = group(pgrid, "graded", (3, 2), 1, env=env, **CG)
        out = run_rhs(R, probs, ref["S"], timers, "slab")
        dv, de = check_rhs(f"{rc.grid_id(pgrid)} slab {switch[4:]}=0", glob, probs, out, ref, (3, 2), timers)
        d = rel_err(dv, dv0), rel_err(de, de0)
        print(f"FIG switch {rc.grid_id(pgrid)} {switch[4:]}=0 timers {timers}: against the default dv {d[0]:.2e} de {d[1]:.2e} "
              f"identical {np.array_equal(dv, dv0)} {np.array_equal(de, de0)}")


# ---- (e) the energy solve in lockstep -----------------------------------------------------------------------------------------------
LOCKSTEP_CASES = [((2, 1, 1), "1"), ((2, 2, 2), "1"), ((3, 1, 1), "1"), ((2, 1, 1), "0"), ((2, 2, 2), "0")]


@pytest.mark.parametrize("pgrid,lockstep", LOCKSTEP_CASES, ids=[f"{rc.grid_id(g)}-lockstep{l}" for g, l in LOCKSTEP_CASES])
def test_energy_solve_in_lockstep(pgrid, lockstep, monkeypatch):
    """One communicator (LGH_COMM2=0), timers off, slab form: two right-hand sides on two different states on fresh contexts.
    The first velocity solve only decides the mode (the first energy solve of a context is sequential); the SECOND
    right-hand side is held to check_rhs against the oracle.  On the all-pairs grids every rank must report a solve that
    ran in lockstep (ready, solves >= 1, iterations inside the velocity solve); with LGH_ENERGY_LOCKSTEP=0 none.  On
    3 x 1 x 1, which is not all-pairs, halo_can_piggyback() is false on every rank, so vcg_mode leaves rz_words and with it
    ls_mine false, vcg_mode_collective's minimum gives rz_words_all = ls_all = 0 and ls_ready stays 0:
    energy_lockstep_capable() is false and the energy solve is the deferred, sequential one - all four statistics are 0."""
    env = {"LGH_VCG_VARIANT": "4", "LGH_COMM2": "0"}
    if lockstep == "0":
        env["LGH_ENERGY_LOCKSTEP"] = "0"
    env = _env(monkeypatch, env)
    refs = [oracle_rhs(pgrid, (3, 2), seed=s) for s in (22, 21)]
    _close_group()
    glob, probs, R = group(pgrid, "graded", (3, 2), 1, env=env, **CG)
    out = run_rhs(R, probs, [r["S"] for r in refs], 0, "slab")
    stats = [x["ls"] for x in out]
    print(f"FIG lockstep {rc.grid_id(pgrid)} LGH_ENERGY_LOCKSTEP={lockstep}: {stats[0]}")
    check_rhs(f"{rc.grid_id(pgrid)} slab COMM2=0 ENERGY_LOCKSTEP={lockstep}", glob, probs, out, refs[1], (3, 2), 0)
    if not rc.ALL_PAIRS_3D[pgrid]:
        assert all(s == dict(solves=0, inside=0, after=0, ready=0) for s in stats), stats
    elif lockstep == "1":
        assert all(s["ready"] == 1 and s["solves"] >= 1 and s["inside"] > 0 for s in stats), stats
    else:
        assert all(s["solves"] == 0 for s in stats), stats
    _close_group()


# ---- (f) another numbering on ranks --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order_multi", [None, "0"], ids=["own-order", "callers-order"])
def test_rhs_on_renumbered_ranks(order_multi, monkeypatch):
    """2 x 2 x 2 ranks, slab form, every rank's block under helpers.PermutedProblem with a seed of its own and the neighbour
    lists translated (rank_cases.permuted_rank): the right-hand side, taken back to the generator's numbering, to check_rhs
    against the oracle.  In the library's own order (the default: the exchange's node lists go through HaloNodeAlias, and
    the slab K1 must find the chains of the structured block again) and in the caller's (LGH_ORDER_MULTI=0: no chain
    survives the renumbering)."""
    pgrid, order = (2, 2, 2), (3, 2)
    env = dict(FORM_ENV["slab"])
    if order_multi is not None:
        env["LGH_ORDER_MULTI"] = order_multi
    env = _env(monkeypatch, env)
    ref = oracle_rhs(pgrid, order)
    glob, probs, R = group(pgrid, "graded", order, 1, env=env, perm_seed=31, **CG)
    assert all(hasattr(p, "node_perm") for p in probs)
    for timers in (0, 1):
        out = run_rhs(R, probs, ref["S"], timers, "slab", extra=lambda ctx: ctx.test_vcg_merged_faces()[1])
        check_rhs(f"{rc.grid_id(pgrid)} slab renumbered ORDER_MULTI={order_multi}", glob, probs, out, ref, order, timers)
        want = sc.n_merged(rc.block_of(pgrid)) if order_multi is None else 0   # (the chains of the structured block, or none)
        assert [x["extra"] for x in out] == [want] * len(probs), [x["extra"] for x in out]
    _close_group()
