"""The quadrature update skips two pieces of work whose result it proves unused before computing it (LGH_Q_DISCARD,
lgh_qpoint.hpp / lgh_qrows.hpp): the dt candidate of a wavefront that cannot lower the folded minimum, and the F.1 rows
of a zone all of whose outputs the flush below eps^2 replaces by +0.0.  The claim is that no output changes a bit, on
any state.  So every state here is run through two contexts that differ in LGH_Q_DISCARD alone, and stressJinvT, the
F.1 E-vector, F^T v and the folded dt estimate are compared as uint64 (the sign of a zero counts); the same results are
held to the project's 1e-12 against the oracle (stress and the two products relative to their largest entry, dt
relative to itself).

States, on the small non-uniform meshes of test_gpu_qupdate_edges.py (12 zones in 3D, 15 in 2D), the mesh undeformed
unless noted (there the viscosity's length scale does not depend on the direction the eigen-decomposition or its
shortcut picks, and parity with the oracle is well defined):
  (a) one zone with e = 1, the rest e = 0; v a tail field of +-1e-40 ... 1e-322 (denormals included) that is exactly zero
      on the nodes of one far zone - hot zone first, middle and last in zone order;
  (b) two updates without a fold between them, the second state's minimum above, equal to and below the first's, with
      the estimate at +inf and at a finite value below and above both beforehand;
  (c) one inverted zone (det J < 0 inside it) with e = 0 and v = 0, a hot zone elsewhere for the oracle's scale;
  (d) all zones the same still state, e scaled by 1 + k 1e-3 in zone k: every candidate inside the bound's slack;
  (e) e = 10^-k, k = 0, 2 ... 44 on still zones: |F.1| crosses eps^2 = 4.9e-32;
  (f) the constant C_F of the F.1 bound against the L1 operator norm of the three back-contractions, by brute force.
That the skips do fire (and do not fire without viscosity) is read from the traced instantiation at Q3Q2.

What fires by construction, confirmed on the CPU with the oracle before the first GPU run:
  * (a): the far zone has e = 0 and v = 0 at all its nodes, so S = 0 and visc_coeff = 0 at all its points (the oracle's
    stress is exactly zero there): its four wavefronts take the `candidate is +inf` skip whatever the hint word holds.
    The wavefront that holds the smallest candidate can never skip (its bound would have to lie above a value that is
    at least the minimum, which is its own candidate); it sits in the hot zone (the oracle's stress is non-zero there).
  * (e): the oracle's max|stressJinvT| of a zone is 1.0e-3 ... 1.5e-3 at k = 0 (3D Q3Q2) and scales with e; C_F = 3 cG cB^2 =
    332.7 there, so the rows are skipped where max|stress| < eps^2 / (2 C_F) = 7.4e-35: in every zone from k = 32 on
    (1.5e-35), in none up to k = 30 (1.0e-33).  (3D Q2Q1: 2.8e-3 ... 4.2e-3, C_F = 150.6, 1.6e-34: the same two k.)
"""
import numpy as np
import pytest

from helpers import make_gpu, make_oracle, rel_err

pytestmark = pytest.mark.gpu

BREAKS3 = [[0, .3, .7, 1], [0, .5, 1], [0, .4, 1]]          # 12 zones
BREAKS2 = [[0, .2, .5, .7, .9, 1], [0, .3, .6, 1]]          # 15 zones
EPS2 = 2.220446049250313e-16 ** 2


def _cfg(id, dim, order, problem=1, env=None):
    return dict(id=id, dim=dim, order=order, problem=problem, env=env or {})


CONFIGS = [
    _cfg("3D-Q3Q2-OCC4=0", 3, (3, 2), env={"LGH_Q_OCC4": "0"}),      # row form, the 144-register build
    _cfg("3D-Q3Q2-OCC4=1", 3, (3, 2), env={"LGH_Q_OCC4": "1"}),      # row form, the 128-register build (the default here)
    _cfg("3D-Q3Q2-FORM=0", 3, (3, 2), env={"LGH_Q_FORM": "0"}),      # point form: only the `candidate is +inf` skip
    _cfg("3D-Q2Q1", 3, (2, 1)),
    _cfg("2D-Q3Q2", 2, (3, 2)),
    _cfg("3D-Q3Q2-problem0", 3, (3, 2), problem=0),                  # no viscosity: nothing may fire
]
IDS = [c["id"] for c in CONFIGS]


def _problem(cfg):
    from oracle.fem import Problem
    return Problem(breaks=BREAKS3 if cfg["dim"] == 3 else BREAKS2, order_v=cfg["order"][0], order_e=cfg["order"][1],
                   problem=cfg["problem"])


def _gpu(prob, env):
    """a device operator whose context read `env` at its creation (the switches are read once per context)"""
    mp = pytest.MonkeyPatch()
    try:
        for k, v in env.items():
            mp.setenv(k, v)
        return make_gpu(prob)
    finally:
        mp.undo()


class Trio:
    """one configuration: the problem, the oracle, and two device operators that differ in LGH_Q_DISCARD alone"""

    def __init__(self, cfg):
        self.cfg = cfg
        self.prob = _problem(cfg)
        self.o = make_oracle(self.prob)
        self.g1 = _gpu(self.prob, dict(cfg["env"], LGH_Q_DISCARD="1"))
        self.g0 = _gpu(self.prob, dict(cfg["env"], LGH_Q_DISCARD="0"))
        assert self.g1.ctx.qupdate_discard()[0] == 3 and self.g0.ctx.qupdate_discard()[0] == 0

    def close(self):
        self.g1.close()
        self.g0.close()
        self.o.close()


class _Trios:
    def __init__(self):
        self.cur = None

    def get(self, cfg_id):
        if self.cur is None or self.cur.cfg["id"] != cfg_id:
            self.close()
            self.cur = Trio(next(c for c in CONFIGS if c["id"] == cfg_id))
        return self.cur

    def close(self):
        if self.cur is not None:
            self.cur.close()
            self.cur = None


@pytest.fixture(scope="module")
def trios():
    t = _Trios()
    yield t
    t.close()


# ---- states ---------------------------------------------------------------------------------------------------------
def still_state(prob, e_zone):
    """the undeformed mesh at rest, energy e_zone[z] at every L2 dof of zone z"""
    S = prob.initial_state()[0].copy()
    S[prob.H1V:2 * prob.H1V] = 0.0
    S[2 * prob.H1V:] = np.repeat(np.asarray(e_zone, dtype=float), prob.NL)
    return S


def tail_field(prob, seed, zero_zones):
    """+-10^-u, u uniform in [40, 322]: what the CG spreads over zones the flow has not reached, down to denormals;
    exactly zero on every node of `zero_zones`"""
    rng = np.random.default_rng(seed)
    v = rng.choice([-1.0, 1.0], prob.H1V) * 10.0 ** (-rng.uniform(40.0, 322.0, prob.H1V))
    v[::7] = rng.choice([-1.0, 1.0], v[::7].size) * 1e-40          # (the scale of the field is 1e-40 in every zone)
    v[3::11] = 3e-310                                               # (denormals for certain)
    v = v.reshape(prob.dim, prob.N)
    for z in zero_zones:
        v[:, prob.h1map[z]] = 0.0
    return v.reshape(-1)


def far_zone(prob, hot):
    return prob.NE - 1 if hot < prob.NE // 2 else 0


def state_a(prob, hot):
    e = np.zeros(prob.NE)
    e[hot] = 1.0
    S = still_state(prob, e)
    S[prob.H1V:2 * prob.H1V] = tail_field(prob, 11 + hot, [far_zone(prob, hot)])
    return S


def state_c(prob):
    """zone `inv`: its interior nodes reflected about its high x face (they leave the zone: d x / d xi changes sign inside
    it; only this zone is deformed).  e = 0 and v = 0 there, a hot zone at the other end, tails elsewhere."""
    inv, hot = prob.NE // 2, (0 if prob.NE // 2 > 1 else prob.NE - 1)
    e = np.zeros(prob.NE)
    e[hot] = 1.0
    S = still_state(prob, e)
    S[prob.H1V:2 * prob.H1V] = tail_field(prob, 5, [inv])
    x = S[:prob.N]
    nodes = prob.h1map[inv]
    lo, hi = x[nodes].min(), x[nodes].max()
    D = prob.D1D
    idx = np.arange(prob.ND)
    inner = np.ones(prob.ND, dtype=bool)
    for a in range(prob.dim):
        i = (idx // D ** a) % D
        inner &= (i > 0) & (i < D - 1)
    assert inner.any() and lo < hi
    x[nodes[inner]] = 2.0 * hi - x[nodes[inner]]
    return S


def state_d(prob):
    return still_state(prob, 1.0 + 1e-3 * np.arange(prob.NE))


def state_e(prob, k):
    return still_state(prob, np.full(prob.NE, 10.0 ** -k))


# ---- results --------------------------------------------------------------------------------------------------------
def device_results(g, S, pre=np.inf, first=None):
    """stressJinvT, the F.1 E-vector and its sum over shared nodes (3D), F^T v and the folded dt estimate of one update of S
    - after an update of `first` without a fold in between, if given - with the estimate set to `pre` beforehand"""
    import torch
    ctx, p = g.ctx, g.p
    ctx.set_dt_est(float(pre))
    torch.cuda.synchronize()
    for state in ([first] if first is not None else []) + [S]:
        Sd = ctx.to_dev(state)
        ctx.reset_quadrature_data()
        ctx.qupdate(Sd)
        ctx.sync()
    out = {}
    _, f1_ok, ftv_ok = ctx.quadrature_generation()
    assert ftv_ok == 1 and f1_ok == (1 if p.dim == 3 else 0)
    if f1_ok:   # (before stressJinvT is asked for: handing out that pointer discards the fused products)
        fe, f1 = ctx.empty(p.dim * p.NE * p.ND), ctx.empty(p.H1V)
        assert ctx.fused_force_e(fe) and ctx.fused_force_mult(f1)
        ctx.sync()
        out["force_e"], out["f1"] = fe.cpu().numpy(), f1.cpu().numpy()
    ftv = ctx.empty(p.L2V)
    assert ctx.fused_force_mult_transpose(ftv)
    ctx.sync()
    out["ftv"] = ftv.cpu().numpy()
    out["sj"] = np.array(ctx.stressJinvT)
    out["dt"] = np.array([ctx.get_dt_est()])
    return out


def oracle_results(o, S):
    o.reset_time_step_estimate()
    o.qdata_is_current = False
    o.update_quadrature_data(S)
    H1V = o.p.H1V
    return dict(sj=o.stressJinvT.copy(), dt=o.L.lgo_get_dt_est(o.h), f1=o.force_mult(np.ones(o.p.L2V)),
                ftv=o.force_mult_transpose(S[H1V:2 * H1V].copy()))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(r1, r0, what):
    assert r1.keys() == r0.keys()
    for k in r1:
        d = np.flatnonzero(bits(r1[k]) != bits(r0[k]))
        assert d.size == 0, f"{what}: {k} differs in {d.size} entries, first at {d[0]}: {r1[k][d[0]]!r} != {r0[k][d[0]]!r}"


def near_oracle(r, ro, what, dt_expected=None):
    fig = dict(sj=rel_err(r["sj"], ro["sj"]), ftv=rel_err(r["ftv"], ro["ftv"]))
    if "f1" in r:
        fig["f1"] = rel_err(r["f1"], ro["f1"])
    dt, dt_o = float(r["dt"][0]), (ro["dt"] if dt_expected is None else dt_expected)
    if dt_o == 0.0 or dt_o == np.inf:
        fig["dt"] = 0.0 if dt == dt_o else np.inf
    else:
        fig["dt"] = abs(dt - dt_o) / dt_o
    print(f"DISCARD {what}: " + " ".join(f"{k} {v:.2e}" for k, v in fig.items()) + f" dt {dt!r}")
    for k, v in fig.items():
        assert v < 1e-12, f"{what}: {k} is {v:.3e} away from the oracle"
    return fig


def check(trio, S, what, **kw):
    r1, r0 = device_results(trio.g1, S, **kw), device_results(trio.g0, S, **kw)
    same_bits(r1, r0, what)
    return r1


# ---- the tests ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("cfg_id", IDS)
def test_dominant_zone(trios, cfg_id, where):
    trio = trios.get(cfg_id)
    prob = trio.prob
    hot = dict(first=0, middle=prob.NE // 2, last=prob.NE - 1)[where]
    S = state_a(prob, hot)
    ro = oracle_results(trio.o, S)
    # what fires by construction (module docstring), on the oracle's numbers
    sj_o = np.abs(ro["sj"]).reshape(prob.dim ** 2, prob.NE, prob.NQ).max(axis=(0, 2)) if ro["sj"].size else None
    if prob.use_viscosity():
        assert sj_o[far_zone(prob, hot)] == 0.0 and sj_o[hot] > 1e-4 and 0.0 < ro["dt"] < np.inf
    r = check(trio, S, f"{cfg_id} (a) hot zone {where}")
    near_oracle(r, ro, f"{cfg_id} (a) hot zone {where}")


@pytest.mark.parametrize("pre", ["inf", "below", "above"])
@pytest.mark.parametrize("second", ["above", "equal", "below"])
@pytest.mark.parametrize("cfg_id", IDS)
def test_hint_history(trios, cfg_id, second, pre):
    trio = trios.get(cfg_id)
    prob = trio.prob
    S1 = still_state(prob, np.full(prob.NE, 1.0))
    S2 = still_state(prob, np.full(prob.NE, dict(above=0.25, equal=1.0, below=4.0)[second]))   # dt ~ 1 / sqrt(e)
    o1, o2 = oracle_results(trio.o, S1), oracle_results(trio.o, S2)
    d1, d2 = float(device_results(trio.g0, S1)["dt"][0]), float(device_results(trio.g0, S2)["dt"][0])
    assert 0.0 < min(d1, d2) and max(d1, d2) < np.inf
    assert (d2 > d1, d2 == d1, d2 < d1) == (second == "above", second == "equal", second == "below")
    v = dict(inf=np.inf, below=0.5 * min(d1, d2), above=2.0 * max(d1, d2))[pre]
    what = f"{cfg_id} (b) second {second}, estimate {pre} beforehand"
    r = check(trio, S2, what, pre=v, first=S1)
    assert float(r["dt"][0]) == min(v, d1, d2), what     # the min of the two separately folded values (and the estimate)
    near_oracle(r, o2, what, dt_expected=min(v, o1["dt"], o2["dt"]))


@pytest.mark.parametrize("cfg_id", IDS)
def test_inverted_zone(trios, cfg_id):
    trio = trios.get(cfg_id)
    S = state_c(trio.prob)
    ro = oracle_results(trio.o, S)
    assert ro["dt"] == 0.0, "the state has no inverted point"
    r = check(trio, S, f"{cfg_id} (c)")
    assert float(r["dt"][0]) == 0.0 and not np.signbit(r["dt"][0])
    near_oracle(r, ro, f"{cfg_id} (c)")


@pytest.mark.parametrize("cfg_id", IDS)
def test_near_tie(trios, cfg_id):
    trio = trios.get(cfg_id)
    prob = trio.prob
    S = state_d(prob)
    ro = oracle_results(trio.o, S)
    r = check(trio, S, f"{cfg_id} (d)")
    near_oracle(r, ro, f"{cfg_id} (d)")
    # the estimate is the smallest of the zones' own (each zone alone hot enough to count, the others cold: +inf)
    per_zone = []
    for z in range(prob.NE):
        e = np.zeros(prob.NE)
        e[z] = 1.0 + 1e-3 * z
        per_zone.append(float(device_results(trio.g0, still_state(prob, e))["dt"][0]))
    assert float(r["dt"][0]) == min(per_zone)


@pytest.mark.parametrize("cfg_id", IDS)
def test_flush_sweep(trios, cfg_id):
    trio = trios.get(cfg_id)
    prob = trio.prob
    seen = []
    for k in range(0, 45, 2):
        S = state_e(prob, k)
        ro = oracle_results(trio.o, S)
        r = check(trio, S, f"{cfg_id} (e) k = {k}")
        near_oracle(r, ro, f"{cfg_id} (e) k = {k}")
        if "force_e" in r:
            seen.append((k, float(np.abs(r["force_e"]).max())))
    if seen:   # the sweep crosses the flush: whole E-vectors of zeros at its end, none at its start
        print("DISCARD (e) max|F.1|:", " ".join(f"{k}:{m:.1e}" for k, m in seen))
        assert seen[0][1] > EPS2 and seen[-1][1] == 0.0
        assert all(m == 0.0 or m >= EPS2 for _, m in seen)


@pytest.mark.parametrize("cfg_id", ["3D-Q3Q2-OCC4=1", "3D-Q2Q1"])
def test_bound_constant(trios, cfg_id):
    """C_F >= the largest |output| of F.1 over all |stressJinvT w detJ| <= 1: the L1 norm of the output's row of the
    three back-contractions, by brute force from the tables the context was created with"""
    trio = trios.get(cfg_id)
    prob = trio.prob
    mode, C_F = trio.g1.ctx.qupdate_discard()
    B, G = np.abs(np.asarray(prob.B)), np.abs(np.asarray(prob.G))     # (Q, D)
    rows = np.zeros((prob.D1D,) * 3)
    for gd in range(3):
        T = [G if a == gd else B for a in range(3)]
        phi = np.einsum("xa,yb,zc->abcxyz", T[0], T[1], T[2])         # |d_gd phi_(a,b,c)| at the point (x, y, z)
        rows += phi.sum(axis=(3, 4, 5))
    norm = rows.max()
    cB, cG = B.sum(axis=0).max(), G.sum(axis=0).max()
    print(f"DISCARD (f) {cfg_id}: C_F {C_F!r}, L1 norm {norm!r}")
    assert mode == 3 and norm <= C_F and C_F == pytest.approx(3.0 * cG * cB * cB, rel=1e-14)
    assert C_F < 4.0 * norm   # (and not a bound that never fires)


# ---- non-vacuity: the traced instantiation (Q3Q2 row form) -----------------------------------------------------------
def traced(prob, S, path, env=None):
    """(wavefronts per workgroup that skipped their dt candidates, F.1 rows skipped 0 / 1 per workgroup) of one update"""
    g = _gpu(prob, dict(env or {}, LGH_Q_TRACE=str(path), LGH_Q_TRACE_CALL="1"))
    try:
        device_results(g, S)
    finally:
        g.close()
    d = np.loadtxt(path, dtype=np.uint64, ndmin=2)
    assert d.shape == (prob.NE, 17)
    return d[:, 15].astype(int), d[:, 16].astype(int)


def test_skips_fire(tmp_path):
    prob = _problem(CONFIGS[1])
    waves = (prob.NQ + 63) // 64
    hot = prob.NE // 2
    nskip, f1 = traced(prob, state_a(prob, hot), tmp_path / "a.txt")
    print("DISCARD trace (a): dt skipped", nskip.tolist(), "F.1 skipped", f1.tolist())
    assert nskip.max() <= waves and 1 <= nskip.sum() < waves * prob.NE      # some wavefronts skipped, some did not
    # (workgroup -> zone is the library's own order: count, do not index)
    assert (nskip == waves).sum() >= 1                                      # the far zone: all of its wavefronts
    assert (nskip < waves).sum() >= 1                                       # the hot zone: not all of its
    assert f1.sum() >= 1 and f1.sum() < prob.NE                             # cold zones flush, the hot one does not
    rows = {}
    for k in (0, 30, 32, 44):
        _, rows[k] = traced(prob, state_e(prob, k), tmp_path / f"e{k}.txt")
    print("DISCARD trace (e): F.1 skipped", {k: v.tolist() for k, v in rows.items()})
    assert not rows[0].any() and not rows[30].any() and rows[32].all() and rows[44].all()


def test_nothing_fires_without_viscosity(tmp_path):
    prob = _problem(CONFIGS[-1])
    assert not prob.use_viscosity()
    for name, S in (("a", state_a(prob, prob.NE // 2)), ("e", state_e(prob, 44))):
        nskip, f1 = traced(prob, S, tmp_path / f"{name}.txt")
        assert not nskip.any() and not f1.any()
