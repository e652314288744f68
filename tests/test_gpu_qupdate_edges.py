"""The quadrature update (qpoint_body through qrows_kernel / qpoint_kernel) and one right-hand side at the edge states
of tests/edge_states.py, against the oracle and - for the uniform states - against a closed form that owes nothing to
either implementation.  Small non-uniform meshes (a transposed zone width shows), every order and every switch that
selects another build of the point body, the instantiation without viscosity, and problem 7's vorticity coefficient.

The bars are the project's existing ones (test_qupdate, test_hydro_mult, test_kernel_switches): stressJinvT and dt
1e-12, dx/dt 1e-13, dv/dt and de/dt 1e-10 (de/dt 1e-8 at Q5Q4) with both CGs at 1e-14.  Two scales are not the
largest oracle entry, because for some states a block of dS/dt is round-off on both sides and an error relative to
it means nothing:
  * dv/dt is relative to max(max|dv_o|, max|dv_o| of the shear state of the same configuration): the affine
    velocity fields give a stress that is constant per zone and a dv/dt of 1e-14 ... 3e-13 (without viscosity the
    shear state's is round-off as well: Pair.dv_scale);
  * de/dt of `rotation` (and of `shear` without viscosity) is relative to max(max|de_o|, max|de_o| of compress_iso
    of the same configuration): the symmetric gradient (resp. its trace) is round-off there, so stress : grad v is.
Two expectations follow the configuration, not the state alone:
  * without viscosity `all_negative_e` has P = S = 0 and no viscous term: stress = 0 and dt = +inf like `still_cold`;
  * problem 7 has gravity: dv/dt of `still_cold` is the acceleration source, only de/dt is exactly zero.

Measured on an MI355X, worst over the states (stress, dt against the oracle | stress, dt against the closed form):
  3D Q1Q0 1.1e-14 4.6e-16 | 1.1e-14 3.7e-16    Q2Q1 7.7e-15 3.1e-15 | 1.2e-15 4.5e-15    Q3Q2 1.1e-14 4.5e-15 | 3.6e-15 9.2e-15
     Q4Q3 2.0e-14 5.8e-15 | 4.6e-15 8.6e-15    Q5Q4 9.6e-15 1.2e-14 | 4.9e-15 1.3e-14 (the same with LGH_Q_PPT=1)
     Q3Q2 with LGH_Q_OCC4=0 / 1 and the force products unfused: as Q3Q2; LGH_Q_FORM=0 and LGH_JAC0_COMPACT=0 (the point
     form both): 5.0e-15 2.2e-15 | 3.3e-15 5.1e-15;  problem 0: 3.2e-15 1.6e-15
  2D Q1Q0 1.1e-15 3.7e-16 | 6.6e-16 4.5e-16    Q2Q1 1.1e-14 3.0e-15 | 1.1e-15 1.5e-14    Q3Q2 1.7e-14 3.4e-15 | 2.6e-15 1.1e-14
     Q4Q3 2.3e-14 1.8e-14 | 2.7e-15 4.0e-14    problem 7: 1.9e-15 4.4e-15
  dv/dt <= 7.6e-14, de/dt <= 3.2e-13 (Q5Q4; 5.2e-14 below it), dx/dt exact.  No state needed an exception from parity."""
import numpy as np
import pytest

import edge_states as es
from helpers import make_gpu, make_oracle, rel_err

pytestmark = pytest.mark.gpu

BREAKS3 = [[0, .3, .7, 1], [0, .5, 1], [0, .4, 1]]          # 12 zones
BREAKS2 = [[0, .2, .5, .7, .9, 1], [0, .3, .6, 1]]          # 15 zones: ragged against every NEB of the 2D point form


def _cfg(id, dim, order, problem=1, env=None, mesh=None):
    return dict(id=id, dim=dim, order=order, problem=problem, env=env or {}, mesh=mesh)


CONFIGS = [
    _cfg("3D-Q1Q0", 3, (1, 0)), _cfg("3D-Q2Q1", 3, (2, 1)), _cfg("3D-Q3Q2", 3, (3, 2)), _cfg("3D-Q4Q3", 3, (4, 3)),   # row form
    _cfg("3D-Q5Q4", 3, (5, 4)),                                                    # point form, two points per thread
    _cfg("3D-Q3Q2-OCC4=0", 3, (3, 2), env={"LGH_Q_OCC4": "0"}),
    _cfg("3D-Q3Q2-OCC4=1", 3, (3, 2), env={"LGH_Q_OCC4": "1"}),
    _cfg("3D-Q3Q2-FORM=0", 3, (3, 2), env={"LGH_Q_FORM": "0"}),
    _cfg("3D-Q3Q2-JAC0_COMPACT=0", 3, (3, 2), env={"LGH_JAC0_COMPACT": "0"}),
    _cfg("3D-Q3Q2-FUSED=0", 3, (3, 2), env={"LGH_FUSED_FTV": "0", "LGH_FUSED_F1": "0"}),
    _cfg("3D-Q5Q4-PPT=1", 3, (5, 4), env={"LGH_Q_PPT": "1"}),
    _cfg("3D-Q3Q2-problem0", 3, (3, 2), problem=0),                                # VISC = false instantiation
    _cfg("2D-Q1Q0", 2, (1, 0)), _cfg("2D-Q2Q1", 2, (2, 1)), _cfg("2D-Q3Q2", 2, (3, 2)), _cfg("2D-Q4Q3", 2, (4, 3)),
    _cfg("2D-Q3Q2-problem7", 2, (3, 2), problem=7, mesh="rt2D"),                   # vorticity coefficient, gravity
]
CASES = [(c["id"], name) for c in CONFIGS for name in es.state_names(c["dim"])]


class Pair:
    """one configuration: the problem, the device operator, the oracle, and the oracle's results per state (computed
    once, shared by the tests that need them, never modified)"""

    def __init__(self, cfg):
        from oracle.fem import Problem
        self.cfg = cfg
        self.mp = pytest.MonkeyPatch()
        for k, v in cfg["env"].items():   # some switches are read at creation, some at every launch: set for the pair's lifetime
            self.mp.setenv(k, v)
        ok, ot = cfg["order"]
        if cfg["mesh"]:
            self.prob = Problem(mesh=cfg["mesh"], rs=0, order_v=ok, order_e=ot, problem=cfg["problem"])
        else:
            self.prob = Problem(breaks=BREAKS3 if cfg["dim"] == 3 else BREAKS2, order_v=ok, order_e=ot, problem=cfg["problem"])
        # (Bernstein mass of order 3 and 4 without preconditioner: the energy CG needs more than the reference's cap of 300
        #  iterations on these meshes, and an iteration cut off unconverged amplifies every rounding difference - the oracle
        #  then misses 1e-10 against itself under a one-ulp change of the state; let it finish, as test_kernel_switches does)
        self.max_iter = 4000 if cfg["order"][0] >= 4 else 300
        self.g, self.o = make_gpu(self.prob), make_oracle(self.prob)
        self.g.cg_tol = self.o.cg_tol = 1e-14
        self.g.cg_max_iter = self.o.cg_max_iter = self.max_iter
        self._oracle = {}

    def close(self):
        self.g.close()
        self.o.close()
        self.mp.undo()

    def dv_scale(self):
        """an honest O(1) scale for dv/dt of the states whose dv/dt is round-off: max|dv_o| of the shear state of this
        configuration.  Without viscosity the shear state's own dv/dt is round-off too (stress = -P I, constant); there
        the scale is the acceleration a pressure difference of P = (gamma - 1) rho e, e = 1, across the smallest zone
        gives: P / (rho w_min)."""
        prob = self.prob
        if prob.use_viscosity():
            return float(np.abs(self.oracle("shear")[2][prob.H1V:2 * prob.H1V]).max())
        gamma = float(np.min(prob.initial_state()[2]))
        return (gamma - 1.0) / min(np.min(np.diff(b)) for b in prob.breaks)

    def oracle(self, name):
        if name not in self._oracle:
            self._oracle[name] = oracle_results(self.o, es.edge_state(self.prob, name))
        return self._oracle[name]


def oracle_results(o, S):
    """(stressJinvT, dt, dS/dt) of the oracle for the state S"""
    o.reset_time_step_estimate()
    o.qdata_is_current = False
    o.update_quadrature_data(S)
    sj, dt = o.stressJinvT.copy(), o.L.lgo_get_dt_est(o.h)
    dS = np.empty_like(S)
    o.qdata_is_current = False
    o.mult(S, dS)
    return sj, dt, dS


def device_qupdate(g, Sd):
    import torch
    g.reset_time_step_estimate()
    g.reset_quadrature_data()
    torch.cuda.synchronize()
    g.update_quadrature_data(Sd)
    return g.ctx.stressJinvT, g.ctx.get_dt_est()


class _Pairs:
    """the pair of the configuration under test; the previous one is closed (and its switches unset) first"""

    def __init__(self):
        self.cur = None

    def get(self, cfg_id):
        if self.cur is None or self.cur.cfg["id"] != cfg_id:
            self.close()
            self.cur = Pair(next(c for c in CONFIGS if c["id"] == cfg_id))
        return self.cur

    def close(self):
        if self.cur is not None:
            self.cur.close()
            self.cur = None


@pytest.fixture(scope="module")
def pairs():
    p = _Pairs()
    yield p
    p.close()


def check_against_oracle(pair, name, sj, dt, dS):
    """C.1 (1)-(3) for results (sj, dt, dS) of any implementation; returns the measured figures"""
    prob, cfg = pair.prob, pair.cfg
    H1V = prob.H1V
    visc, gravity = prob.use_viscosity(), prob.problem == 7
    sj_o, dt_o, dS_o = pair.oracle(name)
    no_signal = name == "still_cold" or (name == "all_negative_e" and not visc)   # P = S = visc_coeff = 0 at every point
    fig = dict(sj=rel_err(sj, sj_o), dt=0.0)
    # 1. the stress
    assert np.all(np.isfinite(sj))
    assert fig["sj"] < 1e-12
    if no_signal:
        assert not np.any(sj) and not np.any(sj_o)
    # 2. the time-step estimate
    if name == "inverted_layer":
        assert dt == 0.0 and dt_o == 0.0
    elif no_signal:
        assert dt == np.inf and dt_o == np.inf
    else:
        assert 0.0 < dt < np.inf and 0.0 < dt_o < np.inf
        fig["dt"] = abs(dt - dt_o) / dt_o
        assert abs(dt - dt_o) <= 1e-12 * dt_o
    # 3. one right-hand side
    assert np.all(np.isfinite(dS)) and np.all(np.isfinite(dS_o))
    dx, dv, de = dS[:H1V], dS[H1V:2 * H1V], dS[2 * H1V:]
    dx_o, dv_o, de_o = dS_o[:H1V], dS_o[H1V:2 * H1V], dS_o[2 * H1V:]
    fig["dx"] = rel_err(dx, dx_o)
    assert fig["dx"] < 1e-13
    v_scale = max(np.abs(dv_o).max(), pair.dv_scale())
    fig["dv"] = float(np.abs(dv - dv_o).max() / v_scale)
    assert fig["dv"] < 1e-10
    e_scale = np.abs(de_o).max()
    if es.de_is_roundoff(name, visc):
        e_scale = max(e_scale, np.abs(pair.oracle("compress_iso")[2][2 * H1V:]).max())
    fig["de"] = float(np.abs(de - de_o).max() / max(e_scale, 1e-300))
    assert fig["de"] < (1e-8 if cfg["order"] == (5, 4) else 1e-10)
    if no_signal:   # both CGs see b = 0 (the velocity one b = M a with gravity): zeros, not NaN
        assert not np.any(de) and not np.any(de_o)
        if not gravity:
            assert not np.any(dv) and not np.any(dv_o)
    return fig


@pytest.mark.parametrize("cfg_id,name", CASES)
def test_edge_state(pairs, cfg_id, name):
    import torch
    pair = pairs.get(cfg_id)
    prob, g, cfg = pair.prob, pair.g, pair.cfg
    S = es.edge_state(prob, name)
    Sd = g.ctx.to_dev(S)
    sj, dt = device_qupdate(g, Sd)
    dS = g.ctx.zeros(S.size)
    torch.cuda.synchronize()
    g.reset_quadrature_data()
    g.mult(Sd, dS)
    g.ctx.sync()
    dS = dS.cpu().numpy()
    sj_o, dt_o, _ = pair.oracle(name)
    print(f"EDGE {cfg_id} {name}: sj {rel_err(sj, sj_o):.2e} dt_g {dt!r} dt_o {dt_o!r}")
    fig = check_against_oracle(pair, name, sj, dt, dS)
    print(f"EDGE {cfg_id} {name}: " + " ".join(f"{k} {v:.2e}" for k, v in fig.items()))

    # 4. the wave-uniform shortcut of the eigen-decomposition claims the bits of the full path for exact-zero gradients
    if cfg["dim"] == 3 and prob.use_viscosity() and name in ("still_hot", "still_cold", "half_still", "still_deformed"):
        try:
            g.ctx.qupdate_set_tiny_grad(-1.0)
            sj_off, dt_off = device_qupdate(g, Sd)
        finally:
            g.ctx.qupdate_set_tiny_grad(1e-30)
        assert np.array_equal(sj_off, sj)
        assert dt_off == dt

    # C.2: the closed form (Sedov configurations: rho0 = 1, gamma = 1.4; h0 from the oracle's operator, which
    # test_setup_data pins the device's to).  It agrees with the oracle to <= 2.8e-15 (stress) and <= 1.5e-14 (dt); the
    # device is held to the same 1e-12 as against the oracle - the four orders left are the kernel's, not the formula's.
    if cfg["problem"] == 1 and name in es.CLOSED_FORM_STATES:
        sj_c, dt_c = es.closed_form(prob, name, pair.o.h0)
        print(f"EDGE {cfg_id} {name}: closed form sj {rel_err(sj, sj_c):.2e} dt {abs(dt - dt_c) / dt_c:.2e}"
              f" (oracle {rel_err(sj_o, sj_c):.2e} {abs(dt_o - dt_c) / dt_c:.2e})")
        assert rel_err(sj_o, sj_c) < 1e-12 and abs(dt_o - dt_c) <= 1e-12 * dt_c
        assert rel_err(sj, sj_c) < 1e-12
        assert abs(dt - dt_c) <= 1e-12 * dt_c
