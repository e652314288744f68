"""lgh_sample_derived (Context.sample_derived): det J, grad v, div v, vorticity and the sound speed on the visualisation
lattice against the numpy restatement of tests/derived_ref.py, on the states, shapes and orders of
tests/test_gpu_sample.py (curved mesh, random v and e with negative values, a random gamma per zone; the 0.2 hmin
displacement already inverts a few points of the cubic meshes).

Tolerance, TOL = 1e-13, the project's figure for sums of at most D1D^dim <= 125 products.  With A_J, A_V
the contractions of J = dx/dxi and V = dv/dxi done with the absolute values of tables and dofs, per lattice point
    |L - L_ref|_F      <= TOL ((|A_V|_F + |L_ref|_F |A_J|_F) |J^-1|_F + kappa_F(J) |L_ref|_F)
    |detJ - detJ_ref|  <= TOL |A_J|_F |J^-1|_F |detJ_ref|
(tests/test_derived_ref.py holds the reference itself to a quarter of it against long double).  div v, the vorticity and
the sound speed are held to EXACT relations on the GPU's own numbers instead."""
import numpy as np
import pytest

from derived_ref import TOL, affine_velocity, derived_reference, lattice_tables3
from test_gpu_sample import CASES, R1S, ZONES, Case

pytestmark = pytest.mark.gpu

NAMES = ("detj", "grad_v", "div_v", "vorticity", "sound_speed")


def names(dim):
    return tuple(k for k in NAMES if dim > 1 or k != "vorticity")


def ncomp(k, dim):
    return {"grad_v": dim * dim, "vorticity": 3 if dim == 3 else 1}.get(k, 1)


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(zones_id, order, renumber=None):
        key = (zones_id, order, renumber)
        if key not in made:
            c = made[key] = Case(ZONES[zones_id], order[0], order[1], renumber)
            c._dref = {}
        return made[key]
    yield get
    for c in made.values():
        c.close()


def reference(c, R1, S=None):
    if S is None and R1 in c._dref:   # computed once, shared, never written
        return c._dref[R1]
    T = lattice_tables3(c.ok, c.ot, R1 - 1)
    ref = derived_reference(c.dim, c.NE, c.N, c.D, c.L, c.h1map, c.S if S is None else S, c.gamma, *T)
    for a in ref.values():
        a.setflags(write=False)
    if S is None:
        c._dref[R1] = ref
    return ref


def derived(c, R1, want=None, Sd=None):
    """dict name -> numpy array of the outputs asked for (the others are passed as NULL), shaped as the reference's"""
    want = names(c.dim) if want is None else want
    NP = c.NE * R1 ** c.dim
    Bh, Gh, Bl = lattice_tables3(c.ok, c.ot, R1 - 1)
    out = {k: c.ctx.to_dev(np.full(ncomp(k, c.dim) * NP, np.nan)) for k in want}   # NaN-filled: an unwritten entry shows
    c.ctx.sample_derived(c.Sd if Sd is None else Sd, Bh, Gh, Bl, **out)
    c.ctx.sync()
    shape = lambda k: (ncomp(k, c.dim), NP) if (k == "grad_v" or (k == "vorticity" and c.dim == 3)) else (NP,)
    return {k: t.cpu().numpy().reshape(shape(k)) for k, t in out.items()}


def check_against(got, ref, what=""):
    for k, a in got.items():
        assert np.all(np.isfinite(a)), (what, k, "an entry was not written")
    if "grad_v" in got:
        err = np.sqrt(((got["grad_v"] - ref["grad_v"]) ** 2).sum(0))
        print(f"{what} grad_v: max |L - L_ref|_F / bound {np.max(err / (TOL * ref['bound_L'])):.4f}")
        assert np.all(err <= TOL * ref["bound_L"]), (what, np.max(err / (TOL * ref["bound_L"])))
    if "detj" in got:
        err = np.abs(got["detj"] - ref["detj"])
        print(f"{what} detj: max err / bound {np.max(err / (TOL * ref['bound_det'])):.4f}")
        assert np.all(err <= TOL * ref["bound_det"]), (what, np.max(err / (TOL * ref["bound_det"])))


def check_exact_relations(c, got, R1):
    """div, vorticity and the sound speed from the GPU's own numbers"""
    dim, L = c.dim, got["grad_v"]
    s = L[0].copy()
    for m in range(1, dim):
        s = s + L[m * dim + m]
    assert np.array_equal(got["div_v"], s)
    if dim == 2:
        assert np.array_equal(got["vorticity"], L[2] - L[1])
    elif dim == 3:
        assert np.array_equal(got["vorticity"], np.stack([L[7] - L[5], L[2] - L[6], L[3] - L[1]]))
    e_gpu = c.sample(R1, want=("e",))["e"]
    g = np.repeat(c.gamma, R1 ** dim)
    want = np.sqrt((g * (g - 1.0)) * np.maximum(e_gpu, 0.0))
    assert np.all(np.abs(got["sound_speed"] - want) <= np.spacing(want))
    return e_gpu


@pytest.mark.parametrize("R1", R1S)
@pytest.mark.parametrize("zones_id,order", CASES, ids=[f"{z}-Q{o[0]}Q{o[1]}" for z, o in CASES])
def test_derived_matches_numpy(cases, zones_id, order, R1):
    c = cases(zones_id, order)
    ref = reference(c, R1)
    got = derived(c, R1)
    check_against(got, ref, f"{zones_id} Q{order[0]}Q{order[1]} R1={R1}")
    e_gpu = check_exact_relations(c, got, R1)
    if c.NE >= 12:   # the clamp of the sound speed is in play
        assert (e_gpu < 0).any() and (got["sound_speed"] == 0).any() and (got["sound_speed"] > 0).any()
    # the rest against the reference too, through the entries they are made of: a wrong pairing of entries would pass the
    # exact relations above only if the test restated the same mistake
    assert np.all(np.abs(got["div_v"] - ref["div_v"]) <= c.dim * TOL * ref["bound_L"])
    if c.dim > 1:
        assert np.all(np.abs(got["vorticity"] - ref["vorticity"]) <= 2 * TOL * ref["bound_L"])


def affine(dim):
    rng = np.random.default_rng(60 + dim)
    return rng.uniform(-1, 1, (dim, dim)), rng.uniform(-1, 1, dim)


@pytest.mark.parametrize("zones_id,order,R1", [("1D-257", (3, 2), 3), ("2D-3x2", (4, 3), 6), ("3D-3x2x2", (2, 1), 3), ("3D-5x5x3", (3, 2), 3),
                                               ("3D-3x2x2", (3, 2), 9)])
def test_affine_velocity_on_the_gpu(cases, zones_id, order, R1):
    """v = A x + b at the nodes of the curved mesh: L = A at every point, within the bound"""
    c = cases(zones_id, order)
    dim = c.dim
    A, b = affine(dim)
    S = affine_velocity(c.S, dim, c.N, A, b)
    ref = reference(c, R1, S)
    got = derived(c, R1, want=("grad_v", "div_v") + (("vorticity",) if dim > 1 else ()), Sd=c.ctx.to_dev(S))
    L = got["grad_v"].T.reshape(-1, dim, dim)
    err = np.sqrt(((L - A) ** 2).sum((1, 2)))
    print(f"{zones_id} R1={R1}: max |L - A|_F / bound {np.max(err / (TOL * ref['bound_L'])):.4f}")
    assert np.all(err <= TOL * ref["bound_L"])
    assert np.all(np.abs(got["div_v"] - np.trace(A)) <= dim * TOL * ref["bound_L"])
    if dim == 2:
        assert np.all(np.abs(got["vorticity"] - (A[1, 0] - A[0, 1])) <= 2 * TOL * ref["bound_L"])
    elif dim == 3:
        curl = np.array([A[2, 1] - A[1, 2], A[0, 2] - A[2, 0], A[1, 0] - A[0, 1]])
        assert np.all(np.abs(got["vorticity"] - curl[:, None]) <= 2 * TOL * ref["bound_L"])


@pytest.mark.parametrize("mesh,order", [("square01_quad", (3, 2)), ("cube01_hex", (3, 2))])
def test_an_inverted_layer_has_negative_detj_and_the_formulas_value(mesh, order):
    """edge_states.inverted_layer: the middle x-layer of zones reflected about its centre.  det J < 0 there, and L is what the
    formula gives: nothing looks at the sign.  (Cubic zones: in a quadratic one the neighbour's face node, moved across the layer,
    makes dx/dxi exactly zero at the opposite face, and a singular J tells nothing.)"""
    from edge_states import edge_state
    from helpers import make_gpu
    from oracle.fem import Problem
    prob = Problem(mesh=mesh, rs=1, order_v=order[0], order_e=order[1], problem=1)
    S = edge_state(prob, "inverted_layer")
    g = make_gpu(prob)
    try:
        dim, NE, N, R1 = prob.dim, prob.NE, prob.N, 4
        NP = NE * R1 ** dim
        T = lattice_tables3(order[0], order[1], R1 - 1)
        gamma = prob.initial_state()[2]
        ref = derived_reference(dim, NE, N, prob.D1D, prob.L1D, np.asarray(prob.h1map).reshape(-1), S, gamma, *T)
        out = dict(detj=g.ctx.to_dev(np.full(NP, np.nan)), grad_v=g.ctx.to_dev(np.full(dim * dim * NP, np.nan)))
        g.ctx.sample_derived(g.ctx.to_dev(S), *T, **out)
        g.ctx.sync()
        got = dict(detj=out["detj"].cpu().numpy(), grad_v=out["grad_v"].cpu().numpy().reshape(dim * dim, NP))
        neg = ref["detj"] < 0
        per_zone = neg.reshape(NE, -1)
        assert per_zone.all(1).any() and (~per_zone).all(1).any()      # whole zones inverted, whole zones not
        assert np.array_equal(got["detj"] < 0, neg)
        assert np.abs(ref["grad_v"][:, neg]).max() > 0
        check_against(got, ref, f"{mesh} inverted")
    finally:
        g.close()


@pytest.mark.parametrize("zones_id,order,R1", [("1D-257", (3, 2), 3), ("2D-3x2", (4, 3), 6), ("3D-5x5x3", (3, 2), 3), ("3D-3x2x2", (3, 2), 9)])
def test_every_output_alone_gives_the_same_bits(cases, zones_id, order, R1):
    c = cases(zones_id, order)
    full = derived(c, R1)
    for k in names(c.dim):
        alone = derived(c, R1, want=(k,))
        assert np.array_equal(alone[k], full[k]), k


def test_two_calls_give_identical_bits(cases):
    for zones_id, order, R1 in (("3D-5x5x3", (3, 2), 6), ("1D-257", (2, 1), 2), ("2D-3x2", (3, 2), 9)):
        c = cases(zones_id, order)
        a, b = derived(c, R1), derived(c, R1)
        for k in a:
            assert np.array_equal(a[k], b[k]), (zones_id, k)


@pytest.mark.parametrize("renumber", ["random", "mfem"])
def test_outputs_sit_at_the_callers_zone_ids(cases, renumber):
    """3 x 2 x 2 zones under another numbering of nodes and zones: the outputs are indexed by the caller's zone ids"""
    c = cases("3D-3x2x2", (3, 2), renumber)
    if renumber == "random":
        assert not np.array_equal(c.elem_perm, np.arange(c.NE))
    assert not np.array_equal(c.node_perm, np.arange(c.N))
    for R1 in (3, 6):
        got = derived(c, R1)
        check_against(got, reference(c, R1), f"{renumber} R1={R1}")
        check_exact_relations(c, got, R1)
    # and they are the values of the same zones of the mesh in its lexicographic numbering: zone j is the structured zone
    # elem_perm[j], structured node i is node node_perm[i]
    lex = cases("3D-3x2x2", (3, 2))
    H1V, NL = 3 * c.N, c.L ** 3
    S_lex = np.concatenate([c.S[k * c.N:(k + 1) * c.N][c.node_perm] for k in range(6)]
                           + [c.S[2 * H1V:].reshape(c.NE, NL)[np.argsort(c.elem_perm)].reshape(-1)])
    T = lattice_tables3(3, 2, 2)
    ref = derived_reference(3, lex.NE, lex.N, lex.D, lex.L, lex.h1map, S_lex, c.gamma[np.argsort(c.elem_perm)], *T)
    got = derived(c, 3)
    perm = lambda a: a.reshape(-1, c.NE, 27)[:, c.elem_perm].reshape(a.shape)
    ref_at_ids = {k: perm(ref[k]) for k in ("detj", "grad_v", "bound_L", "bound_det")}
    check_against(got, ref_at_ids, f"{renumber} against the lexicographic mesh")


def test_refused_calls_name_the_argument_and_run_no_kernel(cases):
    from laghos_amd._lib import LghError
    c = cases("3D-3x2x2", (2, 1))
    for R1 in (1, 10):
        out = c.ctx.zeros(c.NE * R1 ** 3)
        Bh, Bl = np.ones((R1, c.D)), np.ones((R1, c.L))
        with pytest.raises(LghError, match="R1"):
            c.ctx.sample_derived(c.Sd, Bh, Bh, Bl, detj=out, sound_speed=out)
        c.ctx.sync()
        assert not out.cpu().numpy().any()   # no kernel ran
    c1 = cases("1D-3", (2, 1))
    Bh, Gh, Bl = lattice_tables3(2, 1, 2)
    vort, detj = c1.ctx.zeros(c1.NE * 3), c1.ctx.zeros(c1.NE * 3)
    with pytest.raises(LghError, match="vort_out"):
        c1.ctx.sample_derived(c1.Sd, Bh, Gh, Bl, detj=detj, vorticity=vort)
    c1.ctx.sync()
    assert not vort.cpu().numpy().any() and not detj.cpu().numpy().any()


def test_derived_leaves_the_operator_and_the_sampler_alone():
    """The quadrature data, its generation counter and the fused force products are untouched: dS/dt of a state is the same
    bits before and after, lgh_quadrature_generation returns the same triple around the call, S is unchanged, and
    lgh_sample_fields gives the same bits before and after."""
    from helpers import deformed_state, make_gpu
    from lattice_ref import lattice_tables
    from oracle.fem import Problem
    prob = Problem(mesh="cube01_hex", rs=1, order_v=3, order_e=2, problem=1)
    g = make_gpu(prob, cg_tol=1e-12)
    try:
        S = deformed_state(prob, seed=5)
        Sd = g.ctx.to_dev(S)

        def rhs():
            dS = g.ctx.zeros(S.size)
            g.reset_quadrature_data()
            g.mult(Sd, dS)
            g.ctx.sync()
            return dS.cpu().numpy()

        R1 = 4
        NP = prob.NE * R1 ** 3
        Bh, Bl = lattice_tables(3, 2, R1 - 1)
        rho = g.compute_density(Sd)

        def sample():
            out = dict(x=g.ctx.zeros(3 * NP), v=g.ctx.zeros(3 * NP), e=g.ctx.zeros(NP), rho=g.ctx.zeros(NP), p=g.ctx.zeros(NP))
            g.ctx.sample_fields(Sd, rho, Bh, Bl, **out)
            g.ctx.sync()
            return {k: t.cpu().numpy() for k, t in out.items()}

        before, fields = rhs(), sample()
        g.update_quadrature_data(Sd)              # quadrature data and fused products of S on hand
        g.ctx.sync()
        triple = g.ctx.quadrature_generation()
        d = g.derived_fields(Sd, R1 - 1)
        assert g.ctx.quadrature_generation() == triple
        assert set(d) == set(NAMES) and all(np.isfinite(a).all() for a in d.values())
        assert np.abs(d["grad_v"]).max() > 0 and d["detj"].min() > 0
        assert np.array_equal(Sd.cpu().numpy(), S)
        after = sample()
        for k in fields:
            assert np.array_equal(after[k], fields[k]), k
        # the data the call must not have touched is used as it stands: no reset in between
        dS = g.ctx.zeros(S.size)
        g.mult(Sd, dS)
        g.ctx.sync()
        assert np.array_equal(dS.cpu().numpy(), before)
        assert np.array_equal(rhs(), before)
        # HydroOperator.derived_fields is the call of the tests above, with the host library's tables
        T = lattice_tables3(3, 2, R1 - 1)
        gamma = prob.initial_state()[2]
        ref = derived_reference(3, prob.NE, prob.N, prob.D1D, prob.L1D, np.asarray(prob.h1map).reshape(-1), S, gamma, *T)
        check_against(dict(grad_v=d["grad_v"], detj=d["detj"]), ref, "HydroOperator.derived_fields")
    finally:
        g.close()
