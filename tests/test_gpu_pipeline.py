"""GPU parity tests, end to end: the HIP path (through the C ABI) must reproduce
the reference's golden |e| values and agree with the oracle; at BASELINE.json's
full sizes the size-independent properties of the operators are checked."""
import numpy as np
import pytest

import rank_cases as rc
from helpers import deformed_state, make_gpu, rel_err, seeded

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["chk-3D-Sedov", "chk-2D-Sedov", "chk-3D-TG", "chk-2D-TG", "chk-3D-p3", "chk-2D-p3"] +
                         [f"chk-{d}D-p{p}" for p in (2, 4, 5, 6, 7) for d in (3, 2)])
def test_checks_table_on_gpu(golden, name):
    """`--checks` golden values (laghos.cpp:1441-1463) through the HIP path.
    -cgt 1e-14: the CG runs to round-off, so the GPU/CPU difference is the
    accumulated round-off of <= 188 RK4 steps; bar 1e-10 (north_star: 1e-6)."""
    from laghos_amd.hydro import run
    from oracle.fem import Problem
    g = next(c for c in golden["checks"] if c["name"] == name)
    probes = {int(k): v for k, v in g["probes"].items()}
    r = run(Problem(mesh=g["mesh"], rs=0, order_v=2, order_e=1, problem=g["problem"]),
            t_final=0.6, cfl=0.5, cg_tol=1e-14, probe_steps=tuple(probes))
    for step, ref in probes.items():
        got = r["probes"][step]
        assert abs(got - ref) / ref < 1e-10, (name, step, got, ref)


def test_readme_run4_prefix_vs_oracle():
    """3D Sedov Q2Q1 rs2 (README run 4 configuration), first 30 steps, default
    -cgt 1e-8: HIP path vs oracle, |e| and the accepted dt sequence."""
    from laghos_amd.hydro import run
    from oracle.driver import run as orun
    from oracle.fem import Problem
    kw = dict(mesh="cube01_hex", rs=2, problem=1, blast_energy=2.0)
    probes = (5, 10, 20, 30)
    r = run(Problem(**kw), t_final=0.6, max_steps=30, probe_steps=probes)
    o = orun(Problem(**kw), t_final=0.6, max_steps=30, probe_steps=probes)
    for s in probes:
        assert abs(r["probes"][s] - o["probes"][s]) / o["probes"][s] < 1e-7, (s, r["probes"][s], o["probes"][s])


def test_readme_run8_gresho_rk2avg(golden):
    """README run 8 (README.md:222, :234): Gresho vortex, 2D Q3Q2 (kernel 0x246),
    RK2AvgSolver, no artificial viscosity - the only published value at Q3/Q2.
    Same comparison as the reference's `make tests`: step count, printed dt and the
    11 printed digits of |e| (README.md:249-250)."""
    from laghos_amd.hydro import run
    from oracle.fem import Problem
    g = next(c for c in golden["readme"] if c["name"] == "README-8")
    r = run(Problem(mesh=g["mesh"], rs=g["rs"], problem=g["problem"], order_v=g["order_v"], order_e=g["order_e"]),
            t_final=g["tf"], ode_solver=g["ode_solver"])
    assert r["ti"] == g["step"]
    assert f"{r['dt']:.6f}" == g["dt"]
    assert abs(r["e_norm"] - g["e_norm"]) / g["e_norm"] < 5e-11, (r["e_norm"], g["e_norm"])


@pytest.mark.parametrize("name", ["README-1", "README-2", "README-3", "README-4", "README-6", "README-7"])
def test_readme_runs_on_gpu(golden, name):
    """The reference's published verification runs (README.md:214-235; run 3 is BASELINE
    configs[0]) from t = 0 to t_final through the HIP path, compared the way `make tests`
    compares them: final step count, printed dt, |e|.  (Run 8 has its own test below; runs 5
    and 9 are 1D / problem 7 and outside the harness.)"""
    from laghos_amd.hydro import run
    from oracle.fem import Problem
    g = next(c for c in golden["readme"] if c["name"] == name)
    r = run(Problem(mesh=g["mesh"], rs=g["rs"], problem=g["problem"], blast_energy=g["E0"]), t_final=g["tf"])
    assert r["ti"] == g["step"]
    assert f"{r['dt']:.6f}" == g["dt"]
    assert abs(r["e_norm"] - g["e_norm"]) / g["e_norm"] < 1e-9, (r["e_norm"], g["e_norm"])


@pytest.mark.parametrize("ode", [1, 2, 3, 6])
def test_other_rk_integrators_vs_oracle(ode):
    """-s 1 / 2 / 3 / 6 (ForwardEuler, RK2(0.5), RK3SSP, RK6; laghos.cpp:521-525): no published values
    exist for them, so HIP path vs oracle on a short 2D Sedov run, and the C++ driver vs both.  (RK6: Verner's
    tableau has weights of +-176, which amplify the round-off differences of the two paths.)"""
    from laghos_amd import host_lib
    from laghos_amd.hydro import run
    from oracle.driver import run as orun
    from oracle.fem import Problem
    kw = dict(mesh="square01_quad", rs=2, problem=1)
    r = run(Problem(**kw), t_final=0.6, max_steps=12, ode_solver=ode, probe_steps=(12,))
    o = orun(Problem(**kw), t_final=0.6, max_steps=12, ode_solver=ode, probe_steps=(12,))
    assert (r["steps"], r["repeats"]) == (o["steps"], o["repeats"])
    if 12 in o["probes"]:  # (a run that repeats steps does not reach the 12th accepted step in 12 RK steps)
        assert abs(r["probes"][12] - o["probes"][12]) / o["probes"][12] < (1e-9 if ode != 6 else 1e-7)
    assert rel_err(r["S"], o["S"]) < (1e-8 if ode != 6 else 1e-6)
    sim = host_lib.Sim(["-p", 1, "-m", "data/square01_quad.mesh", "-rs", 2, "-ms", 12, "-tf", 0.6, "-s", ode, "-q"])
    while sim.step() == 1:
        pass
    e_cpp, steps_cpp = sim.e_norm(), sim.rk_steps
    sim.close()
    assert steps_cpp == r["steps"]
    assert abs(e_cpp - r["e_norm"]) / r["e_norm"] < 1e-9


def test_q3q2_sedov_vs_oracle():
    """BASELINE config shape (3D Sedov, Q3Q2) at a size the oracle finishes in
    seconds (rs1 = 64 elements): 10 steps, state vector parity."""
    from laghos_amd.hydro import run
    from oracle.driver import run as orun
    from oracle.fem import Problem
    kw = dict(mesh="cube01_hex", rs=1, order_v=3, order_e=2, problem=1)
    r = run(Problem(**kw), t_final=0.6, max_steps=10, cg_tol=1e-12, probe_steps=(10,))
    o = orun(Problem(**kw), t_final=0.6, max_steps=10, cg_tol=1e-12, probe_steps=(10,))
    assert abs(r["probes"][10] - o["probes"][10]) / o["probes"][10] < 1e-9
    assert rel_err(r["S"], o["S"]) < 1e-8
    assert r["steps"] == o["steps"]


@pytest.mark.parametrize("kw", [dict(mesh="cube01_hex", rs=2, order_v=3, order_e=2, problem=1),
                                dict(mesh="cube01_hex", rs=2, order_v=2, order_e=1, problem=0),
                                dict(mesh="box01_hex", rs=1, order_v=2, order_e=1, problem=3),
                                dict(mesh="cube01_hex", rs=1, order_v=1, order_e=0, problem=1),
                                dict(mesh="cube01_hex", rs=1, order_v=4, order_e=3, problem=1)],
                         ids=["sedov-q3q2", "tg-q2q1", "triple-q2q1", "sedov-q1q0", "sedov-q4q3"])
def test_overlapped_energy_solve_is_bit_identical(kw):
    """With the region timers off the hot path takes its fused / overlapped forms: the energy
    solve on a second stream while the velocity solve runs (lgh_solve_energy_begin/_end) and the
    E->L sum of F.1, negation, EliminateRHS, dv = 0 and CG initialisation in one kernel
    (vcg_init_force_k).  Both must give exactly the state of the sequential
    SolveVelocity -> SolveEnergy order with separate kernels: same sums in the same order."""
    from laghos_amd.hydro import run
    from oracle.fem import Problem
    seq = run(Problem(**kw), t_final=0.6, max_steps=12, timers=True)
    ovl = run(Problem(**kw), t_final=0.6, max_steps=12, timers=False)
    assert (seq["steps"], seq["ti"]) == (ovl["steps"], ovl["ti"])
    assert seq["dt"] == ovl["dt"]
    assert np.array_equal(seq["S"], ovl["S"])


@pytest.fixture(scope="module")
def full_size():
    """BASELINE configs[1]: 3D Sedov cube01_hex -rs 4 -ok 3 -ot 2 (32768 elements)"""
    from oracle.fem import Problem
    prob = Problem(mesh="cube01_hex", rs=4, order_v=3, order_e=2, problem=1)
    g = make_gpu(prob)
    yield prob, g
    g.close()


def test_full_size_properties(full_size):
    """Size-independent properties at the full benchmark size:
    adjoint identity of F, symmetry and positivity of M, CG residual, mass of 1."""
    import torch
    prob, g = full_size
    ctx = g.ctx
    sJ = seeded(prob.NE * prob.NQ * 9, 31)
    ctx.set_stressJinvT(sJ)
    e, w = ctx.to_dev(seeded(prob.L2V, 32)), ctx.to_dev(seeded(prob.H1V, 33))
    Fe, Ftw = ctx.empty(prob.H1V), ctx.empty(prob.L2V)
    torch.cuda.synchronize()
    ctx.force_mult(e, Fe)
    ctx.force_mult_transpose(w, Ftw)
    lhs, rhs = ctx.vec_dot(w, Fe), ctx.vec_dot(Ftw, e)
    assert abs(lhs - rhs) <= 1e-11 * max(abs(lhs), abs(rhs))
    # mass: symmetry x.(M y) = y.(M x); (1, M 1) = total mass = volume * rho0 = 1
    x, y = ctx.to_dev(seeded(prob.N, 34)), ctx.to_dev(seeded(prob.N, 35))
    Mx, My = ctx.empty(prob.N), ctx.empty(prob.N)
    torch.cuda.synchronize()
    ctx.mass_set_ess(-1)
    ctx.mass_mult(0, x, Mx)
    ctx.mass_mult(0, y, My)
    a, b = ctx.vec_dot(y, Mx), ctx.vec_dot(x, My)
    assert abs(a - b) <= 1e-11 * max(abs(a), abs(b))
    one = torch.ones(prob.N, dtype=torch.float64, device=ctx.device)
    M1 = ctx.empty(prob.N)
    torch.cuda.synchronize()
    ctx.mass_mult(0, one, M1)
    assert abs(ctx.vec_dot(one, M1) - 1.0) < 1e-12
    # CG: residual of the returned solution
    bvec = ctx.to_dev(seeded(prob.N, 36))
    sol = ctx.zeros(prob.N)
    torch.cuda.synchronize()
    it = ctx.cg_solve(0, bvec, sol, 1e-10, 300)
    assert 0 < it < 300
    r = ctx.empty(prob.N)
    ctx.mass_mult(0, sol, r)
    ctx.sync()
    res = (r - bvec)
    assert float(res.norm() / bvec.norm()) < 1e-8


def test_full_size_sedov_steps(full_size):
    """A few real Sedov steps at full size: energy conservation (the reference
    prints 'Energy diff', laghos.cpp:956-962) and positivity of dt."""
    import torch
    from laghos_amd.hydro import TimeLoop
    prob, g = full_size
    g.reset_quadrature_data()
    loop = TimeLoop(g, t_final=0.6, max_steps=3)
    H1V = prob.H1V
    e0 = g.ctx.internal_energy(loop.S[2 * H1V:]) + g.ctx.kinetic_energy(loop.S[H1V:2 * H1V])
    while loop.step():
        pass
    e1 = g.ctx.internal_energy(loop.S[2 * H1V:]) + g.ctx.kinetic_energy(loop.S[H1V:2 * H1V])
    assert loop.dt > 0 and np.isfinite(loop.dt)
    assert abs(e1 - e0) / e0 < 1e-4  # cg_tol 1e-8: the reference prints diffs of this order
    assert abs(e0 - 0.125) < 1e-12  # E0/2^dim (laghos.cpp:603-604)


def test_64_cubed_schedules_agree(monkeypatch):
    """64^3 zones of Q3Q2 Sedov (the `c3` leg of the bench; HBM-resident, 8x configs[1]): beyond 16 passes per wavefront
    the slab K1 takes the static interleaved schedule instead of the workgroup queues (launch_vcg_slab).  Both
    accumulate (d, A d) in exact integers and K2's (r, z) likewise, so a step through either must give the same bits -
    and the queued one is what the 32^3 runs pin to the oracle.  One RK4 step plus the step the driver always adds;
    energy conservation as in test_full_size_sedov_steps."""
    from laghos_amd import hydro
    from oracle.fem import Problem
    prob = Problem(mesh="cube01_hex", rs=5, order_v=3, order_e=2, problem=1)
    res = {}
    for dyn in ("auto", "1", "0"):
        if dyn == "auto":
            monkeypatch.delenv("LGH_SLAB_DYN", raising=False)
        else:
            monkeypatch.setenv("LGH_SLAB_DYN", dyn)
        res[dyn] = hydro.run(prob, max_steps=1, timers=False)
    a, q, st = res["auto"], res["1"], res["0"]
    assert a["steps"] == q["steps"] == st["steps"] >= 1
    assert np.array_equal(a["S"], st["S"]), "64^3 dispatches the static schedule"
    assert np.array_equal(q["S"], st["S"]), "exact accumulation: the schedule must not change a bit"
    assert a["dt"] == q["dt"] and a["e_norm"] == q["e_norm"] and np.isfinite(a["e_norm"])


def test_config2_full_size_vs_oracle():
    """BASELINE configs[1] at FULL size against the oracle, not only through size-independent properties: 3 RK4 steps
    of the 32^3 Q3Q2 Sedov problem from t = 0 on both sides (12 stages: QUpdate, both force products, three H1 PCG
    solves and the L2 CG solve each, through the kernels the bench times - slab K1, bounded-grid K2, fused QUpdate -
    and the dt controller).  Same step count, same dt, |e| to 1e-9, every block of the state to 1e-8 of its largest
    entry (the solves stop at cg_tol = 1e-8 on both sides with dot products summed in different orders)."""
    from laghos_amd import hydro
    from oracle.driver import run as oracle_run
    from oracle.fem import Problem
    prob = Problem(mesh="cube01_hex", rs=4, order_v=3, order_e=2, problem=1)
    ro = oracle_run(prob, max_steps=3, probe_steps=(1, 2, 3))
    rg = hydro.run(prob, max_steps=3, probe_steps=(1, 2, 3), timers=False)
    assert rg["steps"] == ro["steps"] >= 3 and rg["repeats"] == ro["repeats"]  # (laghos.cpp:716: the step after max_steps still runs)
    assert abs(rg["dt"] - ro["last"]["dt"]) <= 1e-9 * ro["last"]["dt"]  # (dt follows the state: min over the points of a quotient of state values)
    for ti in (1, 2, 3):
        assert abs(rg["probes"][ti] - ro["probes"][ti]) <= 1e-9 * ro["probes"][ti], ti
    H1V = prob.H1V
    for name, sl in (("x", slice(0, H1V)), ("v", slice(H1V, 2 * H1V)), ("e", slice(2 * H1V, None))):
        assert rel_err(rg["S"][sl], ro["S"][sl]) < 1e-8, name


# ---- the C++ host layer (laghos_amd/host): reference API mirror + driver --------------------
@pytest.mark.parametrize("mesh,prob", [(m, p) for p in range(8) for m in ("data/cube01_hex.mesh", "data/square01_quad.mesh")])
def test_cpp_driver_checks(mesh, prob):
    """`laghos -chk` through the C++ driver: both probe points of the reference's
    --checks table must be hit and match (laghos.cpp:903-926)."""
    from laghos_amd import host_lib
    args = ["-p", prob, "-m", mesh, "-rs", 0, "-cgt", "1.e-14", "-chk", "-q", "-pa"]
    n, arr = host_lib._argv(args)
    assert host_lib.load().laghos_main(n, arr) == 0


def test_cpp_driver_matches_python_driver():
    """Same run through the C++ LagrangianHydroOperator/RK4 (own fem.cpp setup) and
    the Python sequencing of the C ABI (oracle numpy setup): identical kernels and
    order; the 1-D tables differ in the last bit, so agreement is ~1e-12, bar 1e-9."""
    from laghos_amd import host_lib
    from laghos_amd.hydro import run
    from oracle.fem import Problem
    sim = host_lib.Sim(["-p", 1, "-m", "data/cube01_hex.mesh", "-rs", 1, "-ok", 3, "-ot", 2, "-ms", 8,
                        "-tf", 0.6, "-q"])
    while sim.step() == 1:
        pass
    S_cpp = sim.state()
    e_cpp = sim.e_norm()
    steps_cpp, ti_cpp = sim.rk_steps, sim.ti
    sim.close()
    r = run(Problem(mesh="cube01_hex", rs=1, order_v=3, order_e=2, problem=1), t_final=0.6, max_steps=8)
    assert (r["steps"], r["ti"]) == (steps_cpp, ti_cpp)
    assert abs(e_cpp - r["e_norm"]) / r["e_norm"] < 1e-9
    assert rel_err(S_cpp, r["S"]) < 1e-9


def test_cpp_driver_readme_run8(golden):
    """README run 8 through the C++ driver (own fem.cpp setup, RK2AvgSolver of
    laghos_amd/host/laghos_solver.cpp), the command line of README.md:222."""
    from laghos_amd import host_lib
    g = next(c for c in golden["readme"] if c["name"] == "README-8")
    sim = host_lib.Sim(["-p", 4, "-m", "data/square_gresho.mesh", "-rs", 3, "-ok", 3, "-ot", 2,
                        "-tf", 0.62831853, "-s", 7, "-pa", "-q"])
    while sim.step() == 1:
        pass
    e, ti, dt = sim.e_norm(), sim.ti, sim.dt
    sim.close()
    assert ti == g["step"]
    assert f"{dt:.6f}" == g["dt"]
    assert abs(e - g["e_norm"]) / g["e_norm"] < 5e-11, (e, g["e_norm"])


def test_readme_run9_rayleigh_taylor(golden):
    """README run 9 (README.md:223, :235): -p 7 -m rt2D -rs 1 -ok 4 -ot 3 -tf 4: vorticity-scaled
    viscosity, gravity source in SolveVelocity, 2D Q4Q3 (0x258), 2462 RK4 steps - through the
    python driver and the C++ driver.  Unstable flow: |e| within the fixture's e_rel_tol."""
    from laghos_amd import host_lib
    from laghos_amd.hydro import run
    from oracle.fem import Problem
    g = next(c for c in golden["readme"] if c["name"] == "README-9")
    r = run(Problem(mesh=g["mesh"], rs=g["rs"], problem=g["problem"], order_v=g["order_v"], order_e=g["order_e"]),
            t_final=g["tf"])
    assert r["ti"] == g["step"]
    assert f"{r['dt']:.6f}" == g["dt"]
    assert abs(r["e_norm"] - g["e_norm"]) / g["e_norm"] < g["e_rel_tol"], (r["e_norm"], g["e_norm"])
    sim = host_lib.Sim(["-p", 7, "-m", "data/rt2D.mesh", "-rs", 1, "-ok", 4, "-ot", 3, "-tf", 4, "-pa", "-q"])
    while sim.step() == 1:
        pass
    e, ti, dt = sim.e_norm(), sim.ti, sim.dt
    sim.close()
    assert ti == g["step"]
    assert f"{dt:.6f}" == g["dt"]
    assert abs(e - g["e_norm"]) / g["e_norm"] < g["e_rel_tol"], (e, g["e_norm"])


def test_cpp_driver_unknown_kernel():
    """(dim, D1D, Q1D) without a kernel must fail loudly like the reference's
    'Unknown kernel' abort (laghos_assembly.cpp:549-553): -ok 6 -ot 5 has no table entry."""
    import subprocess
    import sys
    code = ("from laghos_amd import host_lib; "
            "host_lib.Sim(['-p',1,'-m','data/cube01_hex.mesh','-rs',0,'-ok',6,'-ot',5,'-q'])")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=".")
    assert p.returncode != 0
    assert "Unknown kernel" in (p.stderr + p.stdout)


def _force_multi_parity(mesh_args):
    import json
    import subprocess
    import sys
    code = ("import json,sys; from laghos_amd import host_lib; "
            "s=host_lib.Sim(['-p',1," + mesh_args + ",'-ms',6,'-tf',0.6,'-q']); "
            "n=0\nwhile s.step()==1: n+=1\n"
            "print(json.dumps(dict(e=s.e_norm(), steps=s.rk_steps, t=s.t)))")
    outs = []
    import os
    for force in ("0", "1"):
        env = dict(os.environ, LGH_FORCE_MULTI=force)
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=".")
        assert p.returncode == 0, (p.stdout[-800:], p.stderr[-1500:])
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert lines, (p.stdout[-800:], p.stderr[-1500:])
        outs.append(json.loads(lines[-1]))
    a, b = outs
    assert a["steps"] == b["steps"]
    assert abs(a["e"] - b["e"]) / a["e"] < 1e-10
    assert abs(a["t"] - b["t"]) / a["t"] < 1e-10


def test_multi_rank_code_path_on_one_gpu():
    """LGH_FORCE_MULTI=1: communicator of size 1, so the multi-GPU sequencing
    (separate E->L gather, halo hook, ncclAllReduce of den / (r,z) / dt on the
    context stream, finish kernels) runs for real on this single-GPU box and must
    reproduce the fused single-rank path."""
    _force_multi_parity("'-m','data/cube01_hex.mesh','-rs',1,'-ok',3,'-ot',2")


def test_multi_rank_code_path_on_one_gpu_2d():
    """... and in 2D (data/square01_quad.mesh -rs 2 -ok 2 -ot 1), where the velocity solve is the scalar CG of lgh_scg.hip, one
    component after the other: its several-rank sequencing over real RCCL, on a communicator of size 1."""
    _force_multi_parity("'-m','data/square01_quad.mesh','-rs',2,'-ok',2,'-ot',1")


def test_rccl_grouped_send_recv_on_this_gpu():
    """The halo transport on real RCCL: grouped ncclSend / ncclRecv on the communicator the
    library creates (size 1 under LGH_FORCE_MULTI=1 - the only peer a one-GPU box has is the
    rank itself).  The pack / combine logic around it is covered with emulated ranks below."""
    import os
    import subprocess
    import sys
    code = ("import ctypes; from laghos_amd import host_lib, _lib; "
            "s=host_lib.Sim(['-p',1,'-m','data/cube01_hex.mesh','-rs',1,'-ok',2,'-ot',1,'-ms',1,'-q']); "
            "d=ctypes.c_double(-1.0); "
            "rc=_lib.load().lgh_test_rccl_self_sendrecv(ctypes.c_void_p(s.L.laghos_sim_context(s.h)), 4097, ctypes.byref(d)); "
            "print('RESULT', rc, d.value)")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, LGH_FORCE_MULTI="1"),
                       cwd=".", timeout=300)
    assert p.returncode == 0, (p.stdout[-800:], p.stderr[-1500:])
    line = next(l for l in p.stdout.splitlines() if l.startswith("RESULT"))
    assert line.split()[1:] == ["0", "0.0"], line


@pytest.mark.parametrize("pgrid", [[2, 1, 1], [2, 2, 2]])
def test_halo_logic_emulated_ranks(pgrid):
    """The shared-node sum of the element-sharded path, with the RCCL transport
    replaced by device copies between several contexts on this one GPU: pack
    kernel, buffer layout, neighbour-list ordering and the canonical (ascending
    rank) combine must reproduce the single-rank mass action and make all copies
    of a shared node bit-identical."""
    import torch
    from laghos_amd.context import Context
    from oracle.fem import Problem
    kw = dict(mesh="cube01_hex", rs=1, order_v=2, order_e=1, problem=1)
    nr = int(np.prod(pgrid))
    ref_p = Problem(**kw)
    probs = [Problem(rank=r, pgrid=pgrid, **kw) for r in range(nr)]

    def make(p):
        S, rho_l2, gamma, rho0_q = p.initial_state()
        c = Context(p.dim, p.NE, p.D1D, p.Q1D, p.L1D, p.N, p.h1map, p.B, p.G, p.Bl, p.W, gamma, p.ess,
                    order_v=p.order_v)
        c.setup_rho0detj0(c.to_dev(S[:p.H1V]), c.to_dev(rho_l2), c.to_dev(rho0_q))
        return c
    ref = make(ref_p)
    # a global field sampled on every rank through the node coordinates
    Xg = ref_p.node_coords()
    f = lambda X: np.sin(3 * X[0]) * np.cos(2 * X[1]) + X[2] ** 2
    xg = ref.to_dev(f(Xg))
    yg = ref.empty(ref_p.N)
    torch.cuda.synchronize()
    ref.mass_set_ess(-1)
    ref.mass_mult(0, xg, yg, full=True)
    ref.sync()
    yg = yg.cpu().numpy()
    key = lambda X: np.round(X * 1e6).astype(np.int64)
    gmap = {tuple(k): i for i, k in enumerate(key(Xg).T)}

    ctxs, ys, nbrs, offs = [], [], [], []
    for r, p in enumerate(probs):
        c = make(p)
        c.test_set_rank(nr, r)
        ranks, lists = p.neighbors()
        c.comm_set_neighbors(ranks, lists)
        y = c.empty(p.N)
        torch.cuda.synchronize()
        c.mass_set_ess(-1)
        c.mass_mult(0, c.to_dev(f(p.node_coords())), y, full=True)  # local sums only (no comm attached)
        c.sync()
        off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(int)
        ctxs.append(c); ys.append(y); nbrs.append((ranks, lists)); offs.append(off)
    # emulate the grouped send/recv: block of neighbour k on rank r -> block of neighbour r on rank k
    # (buffer layout of lgh_comm.hip: block k starts at 3*off_k + 4*k, 4 = room for piggy-backed scalars)
    base = lambda r, k: 3 * int(offs[r][k]) + 4 * k
    size = lambda r: 3 * max(int(offs[r][-1]), 1) + 4 * len(nbrs[r][0])
    sends = []
    for r, c in enumerate(ctxs):
        sb = c.zeros(size(r))
        c.test_halo_pack(ys[r], 1, sb)
        c.sync()
        sends.append(sb)
    for r, c in enumerate(ctxs):
        rb = c.zeros(size(r))
        ranks, lists = nbrs[r]
        for k, peer in enumerate(ranks):
            kk = list(nbrs[peer][0]).index(r)
            n = len(lists[k])
            assert n == len(nbrs[peer][1][kk])
            src = sends[peer][base(peer, kk): base(peer, kk) + n]
            rb[base(r, k): base(r, k) + n] = src
        torch.cuda.synchronize()
        c.test_halo_combine(rb, ys[r], 1)
        c.sync()
    # every rank now holds the full sums: compare with the single-rank result, bitwise across ranks
    seen = {}
    for r, p in enumerate(probs):
        yr = ys[r].cpu().numpy()
        idx = np.array([gmap[tuple(k)] for k in key(p.node_coords()).T])
        assert rel_err(yr, yg[idx]) < 1e-13
        for g, v in zip(idx, yr):
            if g in seen:
                assert seen[g] == v  # bit-identical copies on all sharing ranks
            seen[g] = v
    for c in ctxs + [ref]:
        c.close()


def test_word_exchange_buffer_follows_the_neighbour_count():
    """lgh_comm_set_neighbors called again with MORE neighbours on the same context (a re-partition): the peer buffer of the
    exact word exchange (n_nbr x nwords) must grow with it (round-5 advisor: it was only re-allocated when nwords grew, and the
    exchange then wrote behind it)."""
    from laghos_amd.context import Context
    from oracle.fem import Problem
    p = Problem(mesh="cube01_hex", rs=1, order_v=2, order_e=1, problem=1)
    _, _, gamma, _ = p.initial_state()
    c = Context(p.dim, p.NE, p.D1D, p.Q1D, p.L1D, p.N, p.h1map, p.B, p.G, p.Bl, p.W, gamma, p.ess, order_v=p.order_v)
    try:
        c.test_set_rank(2, 0)
        c.comm_set_neighbors([1], [np.arange(5, dtype=np.int32)])
        assert c.test_word_peers(56) == 56
        c.test_set_rank(8, 0)
        c.comm_set_neighbors(list(range(1, 8)), [np.arange(3, dtype=np.int32)] * 7)
        assert c.test_word_peers(56) == 7 * 56
        assert c.test_word_peers(60) == 7 * 60
        c.test_set_rank(2, 0)
        c.comm_set_neighbors([1], [np.arange(5, dtype=np.int32)])
        assert c.test_word_peers(60) == 60
    finally:
        c.close()


MULTI_RANK_CASES = [
    # (ranks, zones, problem, region timers, (ok, ot), environment)
    (2, (8, 8, 8), 1, 1, (3, 2), {}), (8, (8, 8, 8), 1, 1, (3, 2), {}), (3, (9, 6, 6), 1, 1, (3, 2), {}),
    (4, (8, 8, 4), 7, 1, (3, 2), {}), (2, (8, 8, 8), 1, 0, (3, 2), {}), (8, (8, 8, 8), 1, 0, (3, 2), {}),
    (3, (9, 6, 6), 1, 0, (3, 2), {}),
    # the fallbacks a first run over real RCCL may need: no second channel (the default there), no piggy-backed sums
    (8, (8, 8, 8), 1, 0, (3, 2), {"LGH_COMM2": "0"}),
    (8, (8, 8, 8), 1, 0, (3, 2), {"LGH_HALO_PIGGYBACK": "0"}),
    (2, (8, 8, 8), 1, 0, (3, 2), {"LGH_COMM2": "0", "LGH_HALO_PIGGYBACK": "0"}),
    # the slab form of K1 (the default from 20 000 zones per rank: config 4 has 32 768) on several ranks: its exact
    # accumulators are folded before the exchange (vcg_fold_den), by the last workgroup with LGH_SLAB_DEFER=0
    (8, (8, 8, 8), 1, 0, (3, 2), {"LGH_VCG_VARIANT": "4"}), (3, (9, 6, 6), 1, 1, (3, 2), {"LGH_VCG_VARIANT": "4"}),
    (2, (8, 8, 8), 1, 0, (3, 2), {"LGH_VCG_VARIANT": "4", "LGH_COMM2": "0", "LGH_HALO_PIGGYBACK": "0"}),
    (4, (8, 8, 4), 7, 1, (3, 2), {"LGH_VCG_VARIANT": "4", "LGH_SLAB_DEFER": "0"}),
    # round 5: ranks of 8^3 zones (rows of 8: x-chains, merged E-vector) with (r, z) crossing the ranks as exact accumulator
    # words (all-pairs partitions; one message round, no combine kernel), and the ticketed (r, z) the other partitions keep
    (2, (16, 8, 8), 1, 0, (3, 2), {"LGH_VCG_VARIANT": "4"}), (8, (16, 16, 16), 1, 0, (3, 2), {"LGH_VCG_VARIANT": "4"}),
    (8, (8, 8, 8), 1, 1, (3, 2), {"LGH_VCG_VARIANT": "4"}),
    (8, (8, 8, 8), 1, 0, (3, 2), {"LGH_VCG_VARIANT": "4", "LGH_RZ_LIMBS": "0"}),
    (2, (16, 8, 8), 1, 0, (3, 2), {"LGH_VCG_VARIANT": "4", "LGH_SLAB_MERGE": "0"}),
    # the exchanges with their own pack kernels (default: the shared-node gather and K2 fill the send buffers themselves)
    (8, (8, 8, 8), 1, 0, (3, 2), {"LGH_HALO_FUSED_PACK": "0"}), (3, (9, 6, 6), 1, 1, (3, 2), {"LGH_HALO_FUSED_PACK": "0"}),
    # the high-order forms of K1 / K2 on several ranks (BASELINE config 5 is an 8-GPU Q5Q4 run)
    (8, (4, 4, 4), 1, 0, (4, 3), {}), (8, (4, 4, 4), 3, 0, (5, 4), {}), (2, (4, 4, 2), 3, 1, (5, 4), {"LGH_COMM2": "0"}),
    # round 6: every rank is handed its block in an MFEM-like / a random numbering of nodes and zones (LGH_RENUMBER: `-renumber`
    # for the ranks only; the one-rank reference runs on the generator's numbering) - each rank's velocity solve then runs in
    # the library's own order, the node lists of the exchanges translated (HaloNodeAlias); LGH_ORDER_MULTI=0: in the caller's
    (8, (16, 16, 16), 1, 0, (3, 2), {"LGH_VCG_VARIANT": "4", "LGH_RENUMBER": "mfem"}),
    (2, (16, 8, 8), 1, 0, (3, 2), {"LGH_VCG_VARIANT": "4", "LGH_RENUMBER": "random"}),
    (3, (9, 6, 6), 1, 1, (3, 2), {"LGH_RENUMBER": "random"}), (8, (8, 8, 8), 1, 0, (3, 2), {"LGH_RENUMBER": "mfem", "LGH_HALO_FUSED_PACK": "0"}),
    (4, (8, 8, 4), 7, 1, (3, 2), {"LGH_RENUMBER": "mfem"}), (8, (4, 4, 4), 3, 0, (5, 4), {"LGH_RENUMBER": "random"}),
    (2, (16, 8, 8), 1, 0, (3, 2), {"LGH_VCG_VARIANT": "4", "LGH_RENUMBER": "random", "LGH_ORDER_MULTI": "0"}),
    # round 6: ONE communicator (LGH_COMM2=0: the default over RCCL) - the energy CG runs in lockstep with the velocity CG, its
    # two sums per iteration on the velocity iteration's exchanges (lgh_energy_lockstep_stats; "_lockstep": what the run must
    # report); LGH_ENERGY_LOCKSTEP=0: after the velocity solve, as before.  Problem 7: with the gravity source.
    (2, (16, 8, 8), 1, 0, (3, 2), {"LGH_VCG_VARIANT": "4", "LGH_COMM2": "0", "_lockstep": "1"}),
    (8, (16, 16, 16), 1, 0, (3, 2), {"LGH_VCG_VARIANT": "4", "LGH_COMM2": "0", "_lockstep": "1"}),
    (8, (16, 16, 16), 1, 0, (3, 2), {"LGH_VCG_VARIANT": "4", "LGH_COMM2": "0", "LGH_ENERGY_LOCKSTEP": "0", "_lockstep": "0"}),
    (4, (16, 16, 8), 7, 0, (3, 2), {"LGH_VCG_VARIANT": "4", "LGH_COMM2": "0", "_lockstep": "1"}),
    (2, (16, 8, 8), 1, 0, (3, 2), {"LGH_VCG_VARIANT": "4", "LGH_COMM2": "0", "LGH_RENUMBER": "random", "_lockstep": "1"}),
    (8, (16, 16, 16), 1, 0, (3, 2), {"LGH_VCG_VARIANT": "4", "LGH_COMM2": "0", "LGH_RENUMBER": "mfem", "LGH_HALO_FUSED_PACK": "0", "_lockstep": "0"}),
    (8, (16, 16, 16), 1, 0, (3, 2), {"LGH_VCG_VARIANT": "4", "_lockstep": "0"}),  # (second channel: the energy solve beside the velocity solve)
    (8, (16, 16, 16), 1, 1, (3, 2), {"LGH_VCG_VARIANT": "4", "LGH_COMM2": "0", "_lockstep": "0"}),  # (region timers: sequential semantics)
    # blocks that are no powers of two (tests/shape_cases.py), slab K1: 5 x 3 x 2 per rank - every set a chain, the ranks share
    # an x-face; 7 x 3 x 1 - sets at every offset of a row; 5 x 2 x 2 in a 3 x 1 x 1 partition (not all-pairs); and the two
    # ranks again on one communicator with the energy CG in lockstep
    (2, (10, 3, 2), 1, 0, (3, 2), {"LGH_VCG_VARIANT": "4"}),
    (8, (14, 6, 2), 1, 0, (3, 2), {"LGH_VCG_VARIANT": "4"}),
    (3, (15, 2, 2), 1, 1, (3, 2), {"LGH_VCG_VARIANT": "4"}),
    (2, (10, 3, 2), 1, 0, (3, 2), {"LGH_VCG_VARIANT": "4", "LGH_COMM2": "0", "_lockstep": "1"}),
]
# 2D (a zone tuple of two): the velocity solve is the scalar CG of lgh_scg.hip, once per component, with its own several-rank
# sequencing - no lockstep solver, hence no energy solve in lockstep and no "_lockstep" with LGH_COMM2=0.  Blocks of 13 x 5 zones
# on the six rank grids of tests/rank_cases.py (tests/test_rank_cases.py: laghos::Partition picks exactly these grids), region
# timers off and on; Q2Q1 (the order of BASELINE config 1) and Q4Q3; problem 0 (the one configuration with an energy source),
# problem 7 (gravity through the halo-summed MultFull); problem 3 on the 7 x 3 box ("_size") so that its materials cross the
# rank boundaries - 28 x 12 zones (split 4 x 1 by laghos::Partition: a chain of four) and 28 x 16 (2 x 2); the transport and
# numbering switches
MULTI_RANK_CASES += [(rc.n_ranks(g), rc.global_shape(g), 1, t, (3, 2), {}) for t in (0, 1) for g in rc.RANK_GRIDS]
MULTI_RANK_CASES += [
    (4, rc.global_shape((2, 2)), 1, 0, (2, 1), {}), (4, rc.global_shape((2, 2)), 1, 0, (4, 3), {}),
    (4, rc.global_shape((2, 2)), 0, 0, (3, 2), {}), (3, rc.global_shape((3, 1)), 0, 0, (3, 2), {}),
    (4, rc.global_shape((2, 2)), 7, 0, (3, 2), {}),
    (4, (28, 12), 3, 0, (3, 2), {"_size": "7x3"}), (4, (28, 16), 3, 0, (3, 2), {"_size": "7x3"}),
    (4, rc.global_shape((2, 2)), 1, 0, (3, 2), {"LGH_COMM2": "0"}),
    (4, rc.global_shape((2, 2)), 1, 0, (3, 2), {"LGH_HALO_PIGGYBACK": "0"}),
    (4, rc.global_shape((2, 2)), 1, 0, (3, 2), {"LGH_HALO_FUSED_PACK": "0"}),
    (4, rc.global_shape((2, 2)), 1, 0, (3, 2), {"LGH_RENUMBER": "random"}),
    (4, rc.global_shape((2, 2)), 1, 0, (3, 2), {"LGH_RENUMBER": "mfem"}),
]


@pytest.mark.parametrize("nranks,nel,problem,timers,order,env", MULTI_RANK_CASES,
                         ids=[f"{c[0]}ranks-{'x'.join(map(str, c[1]))}-p{c[2]}-t{c[3]}-Q{c[4][0]}Q{c[4][1]}" + "".join(f"-{k[4:] if k[0] != '_' else k[1:]}={v}" for k, v in c[5].items())
                              for c in MULTI_RANK_CASES])
def test_multi_rank_run_on_one_gpu(nranks, nel, problem, timers, order, env, monkeypatch):
    """The complete multi-rank algorithm (block partition, owner-weighted dot products,
    halo pack / canonical combine, separate-gather CG sequencing with its finish
    kernels, dt / |e| reductions) on ONE GPU: the ranks are contexts driven by one host
    thread each over the in-process loopback communicator (lgh_comm.hip, unique id
    "LGHLOCAL..."), which replaces only the RCCL transport.  Must reproduce the
    single-rank run of the same global problem: same accepted / repeated steps, dt and
    |e| to round-off (the ranks sum shared-node contributions in a different order).
    2 and 2x2x2 ranks are all-pairs neighbours: (d, A d) rides on the halo messages; in the
    3x1x1 partition only the middle rank sees all others, so the (collective) decision
    must fall back to the all-reduce on every rank.  The 4-rank case runs problem 7
    (vorticity-scaled viscosity, gravity source through the halo-summed MultFull).
    timers = 0: region timers off, as in bench.py - the energy solve then runs beside the velocity solve on
    the second stream, with its dot products summed over the ranks on the communicator's second channel.
    A zone tuple of two is a 2D run (-dim 2 -nx -ny -Sx 1 -Sy 1): see the comment above the 2D entries."""
    import ctypes
    import os
    import threading
    from laghos_amd import host_lib
    from laghos_amd import _lib
    for k, v in env.items():
        if k[0] != "_":
            monkeypatch.setenv(k, v)
    size = [int(x) for x in env.get("_size", "x".join("1" * len(nel))).split("x")]
    args = ["-p", problem, "-dim", len(nel)]
    for a in range(len(nel)):   # the dimension is the length of the zone tuple
        args += ["-n" + "xyz"[a], nel[a], "-S" + "xyz"[a], size[a]]
    args += ["-rs", 0, "-ok", order[0], "-ot", order[1], "-pa", "-tf", 0.6, "-ms", 6 if order == (3, 2) else 3, "-q"]
    ref = host_lib.Sim(args)
    ref.enable_timers(timers)
    while ref.step() == 1:
        pass
    want = dict(e=ref.e_norm(), t=ref.t, dt=ref.dt, rk=ref.rk_steps, ti=ref.ti)
    ref.close()

    cid = (b"LGHLOCAL" + os.urandom(16).hex().encode()).ljust(128, b"\0")
    out, err = {}, {}

    def rank_main(rank):
        try:
            rargs = args + (["-renumber", env["LGH_RENUMBER"], "-renumber-seed", 3 + rank] if "LGH_RENUMBER" in env else [])
            sim = host_lib.Sim(rargs, nranks=nranks, rank=rank, nccl_id=cid)
            sim.enable_timers(timers)
            while sim.step() == 1:
                pass
            ls = (ctypes.c_long * 4)()
            _lib.check(_lib.load().lgh_energy_lockstep_stats(sim.L.laghos_sim_context(sim.h), ls))
            out[rank] = dict(e=sim.e_norm(), t=sim.t, dt=sim.dt, rk=sim.rk_steps, ti=sim.ti, ls=list(ls))
            sim.close()
        except Exception as ex:  # noqa: BLE001 - reported below
            err[rank] = repr(ex)

    threads = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(nranks)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=240)
    assert not any(t.is_alive() for t in threads), "a rank did not finish (collective mismatch?)"
    assert not err, err
    for r in range(nranks):
        got = out[r]
        assert (got["rk"], got["ti"]) == (want["rk"], want["ti"]), (r, got, want)
        assert abs(got["dt"] - want["dt"]) <= 1e-12 * want["dt"], (r, got, want)
        # (orders 4 and 5: the unpreconditioned L2 CG on the Bernstein mass matrix amplifies the rounding differences of
        #  the rank-ordered sums - cond ~ 1e6; the README runs themselves are held to 1e-9)
        assert abs(got["e"] - want["e"]) <= (1e-10 if order == (3, 2) else 1e-9) * want["e"], (r, got, want)
        if len(nel) == 2:
            assert got["ls"] == [0, 0, 0, 0], (r, got)   # no lockstep velocity solve in 2D, so no energy solve in lockstep with it
        if "_lockstep" in env:
            solves, inside, after, ready = got["ls"]
            if env["_lockstep"] == "1":
                # every energy solve from the second RK stage on (the first velocity solve of a run has not decided yet how
                # (r, z) crosses the ranks), nearly all of their iterations inside the velocity solves
                assert ready == 1 and solves >= 2 * want["rk"] - 1 and inside > 4 * solves and after <= inside // 4, (r, got)
            else:
                assert solves == 0 and inside == 0, (r, got)
    assert len({(o["e"], o["dt"]) for o in out.values()}) == 1, out  # every rank holds the same numbers, bit for bit


@pytest.mark.parametrize("nranks,nel", [(2, (16, 8, 8)), (8, (16, 16, 16))], ids=["2ranks", "8ranks"])
def test_lockstep_energy_solve_is_bit_identical_to_the_sequential_order(nranks, nel, monkeypatch):
    """One communicator (LGH_COMM2=0), slab K1: the energy CG interleaved with the velocity CG, its (d, M d) on the halo messages
    and its (r, r) in the accumulator-word exchange, forms its sums in the order the all-pairs all-reduce of the sequential order
    forms them (ascending rank) - so the two runs must agree in every bit of |e|, t and dt, on every rank."""
    import ctypes
    import os
    import threading
    from laghos_amd import host_lib, _lib
    monkeypatch.setenv("LGH_VCG_VARIANT", "4")
    monkeypatch.setenv("LGH_COMM2", "0")
    args = ["-p", 1, "-dim", 3, "-nx", nel[0], "-ny", nel[1], "-nz", nel[2], "-Sx", 1, "-Sy", 1, "-Sz", 1, "-rs", 0,
            "-ok", 3, "-ot", 2, "-pa", "-tf", 0.6, "-ms", 5, "-q"]
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("LGH_ENERGY_LOCKSTEP", mode)
        cid = (b"LGHLOCAL" + os.urandom(16).hex().encode()).ljust(128, b"\0")
        out, err = {}, {}

        def rank_main(rank):
            try:
                sim = host_lib.Sim(args, nranks=nranks, rank=rank, nccl_id=cid)
                sim.enable_timers(0)
                while sim.step() == 1:
                    pass
                ls = (ctypes.c_long * 4)()
                _lib.check(_lib.load().lgh_energy_lockstep_stats(sim.L.laghos_sim_context(sim.h), ls))
                out[rank] = (sim.e_norm(), sim.t, sim.dt, sim.rk_steps, ls[0] > 0)
                sim.close()
            except Exception as ex:  # noqa: BLE001 - reported below
                err[rank] = repr(ex)

        th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(nranks)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=240)
        assert not any(t.is_alive() for t in th) and not err, err
        assert len(set(out.values())) == 1, out
        res[mode] = out[0]
    assert res["1"][4] and not res["0"][4]
    assert res["1"][:4] == res["0"][:4], res


def test_lockstep_energy_solve_with_its_own_iteration_cap(monkeypatch):
    """The energy solve in lockstep is interleaved for as many iterations as it needed last time - but never past the cap THIS
    solve was given (lgh_solve_energy_begin's max_iter may be smaller than the velocity solve's): the rest of the sequence must
    be that of the sequential order, bit for bit.  One rank through the N-rank path (communicator of size 1, no second channel)."""
    import ctypes
    import os
    from oracle.fem import Problem
    from laghos_amd import _lib
    for k, v in (("LGH_FORCE_MULTI", "1"), ("LGH_COMM2", "0"), ("LGH_VCG_VARIANT", "4")):
        monkeypatch.setenv(k, v)
    prob = Problem(mesh="cube01_hex", rs=3, order_v=3, order_e=2, problem=1)
    S = deformed_state(prob, seed=5)
    H1V = prob.H1V

    def run(lockstep):
        monkeypatch.setenv("LGH_ENERGY_LOCKSTEP", lockstep)
        g = make_gpu(prob)
        try:
            g.ctx.comm_init(1, 0, (b"LGHLOCAL" + os.urandom(16).hex().encode()).ljust(128, b"\0"))
            ctx = g.ctx
            ctx.enable_timers(False)  # (region timers have sequential semantics: no overlap, no lockstep)
            Sd, dS = ctx.to_dev(S), ctx.zeros(S.size)
            out = []
            for e_cap in (300, 300, 3, 300, 1):
                ctx.vec_copy(dS[:H1V], Sd[H1V:2 * H1V])
                g.reset_quadrature_data()
                g.update_quadrature_data(Sd)
                ctx.solve_energy_begin(Sd, Sd[H1V:2 * H1V], dS, g.e_rhs, 1e-14, e_cap)
                ctx.solve_velocity(Sd, dS, None, g.rhs, g.work, 1e-14, 300)
                ctx.solve_energy_end()
                ctx.sync()
                out.append(dS.cpu().numpy().copy())
            ls = (ctypes.c_long * 4)()
            _lib.check(_lib.load().lgh_energy_lockstep_stats(ctx.h, ls))
            return out, list(ls)
        finally:
            g.close()

    a, sa = run("1")
    b, sb = run("0")
    assert sa[0] == 4 and sa[1] > 8 and sb[0] == 0, (sa, sb)  # (the first solve of a context is sequential)
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), k


def test_cpp_driver_print_dumps(tmp_path):
    """`-print -k <basename>` (laghos.cpp:873-900): basename_<ti>_{mesh,rho,v,e} at every visualisation
    step and at the last one, 8 significant digits; v and e are the blocks of the state vector, the nodes
    of the mesh file its position block."""
    from laghos_amd import host_lib
    base = tmp_path / "out" / "Laghos"
    sim = host_lib.Sim(["-p", 1, "-m", "data/cube01_hex.mesh", "-rs", 1, "-ok", 2, "-ot", 1, "-ms", 3, "-vs", 2, "-tf", 0.6,
                        "-print", "-k", str(base), "-q"])
    while sim.step() == 1:
        pass
    S, last = sim.state(), sim.ti
    sz = sim.sizes()
    sim.close()
    tis = sorted({int(p.name.split("_")[1]) for p in base.parent.glob("Laghos_*_v")})
    assert 2 in tis and last in tis
    for ti in tis:
        for what in ("mesh", "rho", "v", "e"):
            assert (base.parent / f"Laghos_{ti}_{what}").exists()
    H1V = 3 * sz["N"]

    def values(path, header_lines):
        txt = path.read_text().split("\n\n")
        return txt[0], np.array([float(x) for x in txt[-1].split()])
    head, v = values(base.parent / f"Laghos_{last}_v", 5)
    assert "FiniteElementCollection: H1_3D_P2" in head and "VDim: 3" in head and "Ordering: 0" in head
    assert v.size == H1V and np.allclose(v, S[H1V:2 * H1V], rtol=1e-7, atol=1e-300)
    head, e = values(base.parent / f"Laghos_{last}_e", 5)
    assert "FiniteElementCollection: L2_T2_3D_P1" in head
    assert e.size == S.size - 2 * H1V and np.allclose(e, S[2 * H1V:], rtol=1e-7, atol=1e-300)
    head, rho = values(base.parent / f"Laghos_{last}_rho", 5)
    assert rho.size == e.size and rho.min() > 0
    mesh = (base.parent / f"Laghos_{last}_mesh").read_text()
    assert mesh.startswith("LGH mesh v1.0") and f"elements\n{sz['NE']}\n" in mesh
    x = np.array([float(t) for t in mesh.split("\n\n")[-1].split()])
    assert x.size == H1V and np.allclose(x, S[:H1V], rtol=1e-7, atol=1e-12)
