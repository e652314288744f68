"""Kernel-level parity of K2, the node kernel of the lockstep velocity solve and the kernel with the largest share of an RK
step: ONE launch through the C ABI (lgh_test_vcg_k2) in every form the one-rank solve can dispatch - the bounded-grid
kernel with the ticketed fold of (r, z), the same with the exact accumulators (slab K1, element-local and merged
E-vector), one or two nodes per thread, and the round-1 kernel - against ONE ITERATION OF THE ORACLE'S OWN CG LOOP
(oracle/laghos_oracle.cpp::lgo_cg, the restatement of upstream's CGSolver::Mult that tests/test_oracle_golden.py pins to
the reference's --checks table; /root/reference/laghos_solver.cpp:272-283, :383-392): the oracle solves each of the three
component systems M x = b with max_iter = it - 1 and with max_iter = it, and its residual, direction, iterate and
scalars before / after iteration `it` (lgo_cg_vec, lgo_cg_scalars) are the inputs and the expected outputs of the
launch; the E-vector K1 would have written is the oracle's element mass apply of the oracle's direction
(laghos_assembly.cpp:117-121).  No recurrence is restated here (round-4 verdict, weak #2).  Tolerance 1e-13 of the
largest entry.  The bench size (32^3 zones, the default dispatch) is one of the cases."""
import numpy as np
import pytest

from helpers import make_gpu, make_oracle, rel_err, seeded

pytestmark = pytest.mark.gpu

# (id, mesh, rs, order_v, order_e, environment, bounded-grid kernel expected)
K2_CASES = [
    ("Q3Q2-64-default", "cube01_hex", 1, 3, 2, {}, True),
    ("Q3Q2-128-slab-exact-rz", "box01_hex", 1, 3, 2, {"LGH_VCG_VARIANT": "4"}, True),
    ("Q3Q2-128-slab-ticketed-rz", "box01_hex", 1, 3, 2, {"LGH_VCG_VARIANT": "4", "LGH_RZ_LIMBS": "0"}, True),
    ("Q3Q2-512-slab-exact-rz", "cube01_hex", 2, 3, 2, {"LGH_VCG_VARIANT": "4"}, True),
    ("Q3Q2-64-all-slots", "cube01_hex", 1, 3, 2, {"LGH_K2_SKIP": "0"}, True),
    ("Q3Q2-64-round-1-kernel", "cube01_hex", 1, 3, 2, {"LGH_K2P": "0"}, False),
    ("Q2Q1-64-default", "cube01_hex", 1, 2, 1, {}, True),
    ("Q4Q3-16-default", "box01_hex", 0, 4, 3, {}, True),
    ("Q5Q4-16-default", "box01_hex", 0, 5, 4, {}, True),
    ("Q3Q2-128-slab-element-local", "box01_hex", 1, 3, 2, {"LGH_VCG_VARIANT": "4", "LGH_SLAB_MERGE": "0"}, True),
    ("Q3Q2-4096-slab-exact-rz", "cube01_hex", 3, 3, 2, {"LGH_VCG_VARIANT": "4"}, True),   # whole x-chains and sets that straddle rows
]


def _oracle_iteration(prob, o, it, deferred_x):
    """Inputs and expected outputs of K2 in iteration `it` from the oracle's CG (three component solves of M x = b)."""
    from oracle.driver import _dp
    N, NE, ND = prob.N, prob.NE, prob.ND
    hmap = np.asarray(prob.h1map).reshape(NE, ND)
    inp = dict(r=np.zeros(3 * N), d=np.zeros(3 * N), x=np.zeros(3 * N), yE=np.zeros((3, NE * ND)), den=np.zeros(3), rz=np.zeros(3),
               rz_prev=np.ones(3), alpha_prev=np.zeros(3))
    exp = dict(r=np.zeros(3 * N), d=np.zeros(3 * N), x=np.zeros(3 * N), rz=np.zeros(3))
    dinv = 1.0 / np.asarray(o.diagV)
    for c in range(3):
        sl = slice(c * N, (c + 1) * N)
        b = seeded(N, 210 + c)
        ess = np.asarray(prob.ess[c], dtype=np.int64)
        if len(ess):
            b[ess] = 0.0                                      # EliminateRHS (laghos_solver.cpp:386)
        if not np.any(b):
            # every node essential for this component (one zone across an axis at Q1): the oracle's CG returns before its
            # first iteration and leaves no scalars.  The launch still runs on the component: zero vectors with the
            # scalars of a unit step (alpha = rz / den = 1, beta = 0 / 1) must come back as zeros, (r, z) = 0.
            inp["rz"][c] = inp["den"][c] = 1.0
            continue

        def run(m):
            x, _ = o.cg(0, b, x=np.zeros(N), comp=c, rel_tol=0.0, max_iter=m)
            r, d, sc = o.cg_state(0)
            return x, r, d, sc
        x_it, r_it, d_it, sc = run(it)                        # after iteration `it`
        exp["r"][sl], exp["d"][sl], exp["rz"][c] = r_it, d_it, sc[3]
        inp["rz"][c], inp["den"][c] = sc[0], sc[1]
        if it == 1:
            inp["r"][sl] = b                                  # r_0 = b - M 0; no direction, no (r, z) before it
            x_prev = np.zeros(N)
        else:
            x_prev, r_prev, d_prev, sc_prev = run(it - 1)
            inp["r"][sl], inp["d"][sl] = r_prev, d_prev
            inp["rz_prev"][c], inp["alpha_prev"][c] = sc_prev[0], sc_prev[2]
            assert abs(sc_prev[3] - sc[0]) <= 1e-14 * abs(sc[0])  # (r, z) after it - 1 is the nom of iteration it (OpenMP sums: not the same bits twice)
        # the E-vector K1 hands over: the oracle's element mass apply of the oracle's direction of this iteration
        xE = np.ascontiguousarray(d_it[hmap].reshape(-1))
        o.L.lgo_mass_apply_E(o.h, 0, _dp(xE), _dp(inp["yE"][c]))
        if deferred_x:
            if it % 2 == 0:
                # the bounded-grid kernel holds x of two iterations ago and adds both terms (it = 2: the old content is not read)
                inp["x"][sl] = run(it - 2)[0] if it > 2 else seeded(N, 230 + c)
                exp["x"][sl] = x_it
            else:
                inp["x"][sl] = x_prev                         # untouched by an odd launch
                exp["x"][sl] = x_prev
        else:
            inp["x"][sl], exp["x"][sl] = x_prev, x_it
    return inp, exp


@pytest.mark.parametrize("it", [1, 2, 3, 4], ids=lambda i: f"it{i}")
@pytest.mark.parametrize("case", K2_CASES, ids=[c[0] for c in K2_CASES])
def test_k2_one_launch_vs_oracle_cg(case, it, monkeypatch):
    from oracle.fem import Problem
    _, mesh, rs, ok, ot, env, bounded = case
    for k in ("LGH_VCG_VARIANT", "LGH_RZ_LIMBS", "LGH_K2_SKIP", "LGH_K2P", "LGH_SLAB_MERGE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prob = Problem(mesh=mesh, rs=rs, order_v=ok, order_e=ot, problem=1)
    _run_k2(prob, it, bounded, "slab" if "LGH_VCG_VARIANT" in env else None)


def _run_k2(prob, it, bounded, form):
    g, o = make_gpu(prob), make_oracle(prob)
    try:
        if form is not None:
            assert g.ctx.k1_form() == form
        inp, exp = _oracle_iteration(prob, o, it, bounded)
        rd, dd, xd = g.ctx.to_dev(inp["r"]), g.ctx.to_dev(inp["d"]), g.ctx.to_dev(inp["x"])
        rz_g, deferred = g.ctx.test_vcg_k2(it, g.ctx.to_dev(np.ascontiguousarray(inp["yE"].reshape(-1))), rd, dd, xd, inp["den"], inp["rz"],
                                            inp["rz_prev"], inp["alpha_prev"])
        assert deferred == bounded
        r_g, d_g, x_g = rd.cpu().numpy(), dd.cpu().numpy(), xd.cpu().numpy()
    finally:
        g.close()
        o.close()
    tol = 1e-13
    print(f"FIG k2 it {it} r {rel_err(r_g, exp['r']):.2e} d {rel_err(d_g, exp['d']):.2e} x {rel_err(x_g, exp['x']):.2e}"
          f" rz {max(abs(rz_g[c] - exp['rz'][c]) / max(abs(exp['rz'][c]), 1e-300) for c in range(3)):.2e}")
    assert rel_err(r_g, exp["r"]) < tol, "r"
    assert rel_err(d_g, exp["d"]) < tol, "d"
    assert rel_err(x_g, exp["x"]) < tol, "x"
    for c in range(3):
        assert abs(rz_g[c] - exp["rz"][c]) <= tol * abs(exp["rz"][c]), (c, "(r, z)", rz_g[c], exp["rz"][c])


@pytest.mark.parametrize("it", [2, 3], ids=lambda i: f"it{i}")
def test_k2_at_bench_size_vs_oracle_cg(it, monkeypatch):
    """Config 2's mesh (32^3 zones, Q3Q2) as dispatched by default: slab K1 (merged E-vector layout), exact (r, z)
    accumulators, bounded-grid K2 - the launch the bench's roofline is quoted on - against the oracle's CG iteration."""
    from oracle.fem import Problem
    for k in ("LGH_VCG_VARIANT", "LGH_RZ_LIMBS", "LGH_K2_SKIP", "LGH_K2P", "LGH_SLAB_MERGE"):
        monkeypatch.delenv(k, raising=False)
    prob = Problem(mesh="cube01_hex", rs=4, order_v=3, order_e=2, problem=1)
    _run_k2(prob, it, True, "slab")


EXACT_CASES = [("Q3Q2-16-slab", "box01_hex", 0), ("Q3Q2-512-slab", "cube01_hex", 2)]


@pytest.mark.parametrize("case", EXACT_CASES, ids=[c[0] for c in EXACT_CASES])
def test_k2_rz_out_of_the_window(case, monkeypatch):
    """The exact accumulators of (r, z) (slab K1, bounded-grid K2) with rz of the iteration before understated by 2^-60:
    the window lies 60 binades too low, the workgroups' shares of the new (r, z) - which alpha = rz / den, 2^-60 of what it
    should be, leaves at the size of the old one - do not fit, and (r, z) must come back NaN in all three components, not
    as a wrong number.  The next launch with the true rz returns the bits of the first: the flag does not outlive the solve."""
    from oracle.fem import Problem
    _, mesh, rs = case
    for k in ("LGH_VCG_VARIANT", "LGH_RZ_LIMBS", "LGH_K2_SKIP", "LGH_K2P", "LGH_SLAB_MERGE"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("LGH_VCG_VARIANT", "4")
    prob = Problem(mesh=mesh, rs=rs, order_v=3, order_e=2, problem=1)
    g, o = make_gpu(prob), make_oracle(prob)
    try:
        assert g.ctx.k1_form() == "slab"
        it = 2
        inp, exp = _oracle_iteration(prob, o, it, True)
        yE = g.ctx.to_dev(np.ascontiguousarray(inp["yE"].reshape(-1)))
        low = 2.0 ** -60
        # the claim: (r, z) of the residual the understated alpha leaves (r itself, to 2^-60) against the understated window -
        # the largest of the workgroups' non-negative shares is at least their mean, and there are fewer workgroups than nodes
        dinv = 1.0 / np.asarray(o.diagV)
        for c in range(3):
            rc = inp["r"][c * prob.N:(c + 1) * prob.N]
            assert float(np.dot(rc * rc, dinv)) / prob.N >= 2.0 ** (np.frexp(inp["rz"][c] * low)[1] + 11)
        out = []
        for f in (1.0, low, 1.0):
            rd, dd, xd = g.ctx.to_dev(inp["r"]), g.ctx.to_dev(inp["d"]), g.ctx.to_dev(inp["x"])
            rz_g, deferred = g.ctx.test_vcg_k2(it, yE, rd, dd, xd, inp["den"], inp["rz"] * f, inp["rz_prev"] * f, inp["alpha_prev"])
            assert deferred
            out.append(rz_g.copy())
    finally:
        g.close()
        o.close()
    for c in range(3):
        assert abs(out[0][c] - exp["rz"][c]) <= 1e-13 * abs(exp["rz"][c])
    assert np.all(np.isnan(out[1])), out[1]
    assert np.array_equal(out[2].view(np.int64), out[0].view(np.int64)), (out[0], out[2])
