"""lgh_profile (Context.profile, Sim.profile): binned 1-D profiles of a state with exact, order-free bin sums, against the numpy
restatement of tests/profile_ref.py, the figures of lgh_diagnostics, and the edge states of tests/edge_states.py.

States and shapes are those of tests/test_gpu_diagnostics.py (its `Case`; tests/profile_cases.py rebuilds the same numbers
without a GPU, and tests/test_profile_ref.py holds every (case, spec) to `undecided == 0` there: no point within 1e-9 of a bin
edge, of detJ = 0 or of the origin - which is what lets the counts be demanded exactly here).

Bounds per row (none taken from what the kernel gives); abs = sum |addend| of the row's points, c = dim D1D^dim + 8:
  n                  exact;
  rho_min, rho_max   relative max(1e-13, 2 eps kappa), the bound of test_gpu_diagnostics.check_zones;
  ie, ke, mxi        c 2^-52 abs: the kernel's sum is exact and numpy's is correctly rounded, so what is left is the addends -
                     each a product of interpolated values of dim D1D^dim terms, formed in another order than numpy's;
  mass               2^-52 abs: the addends are read back bit-exact (Context.rho0DetJ0w), the sum is exact on both sides, the
                     two roundings of the results are left;
  vol, pv            c max(1, kappa) 2^-52 abs: detJ carries the condition of J = sum G x;
  mom                as ie for an axis; along r the direction (x_q - o) / r_q adds 2^-52 sum_q m |v| max |x_q - o|_1 / r_q.
Rows of a handful of points (4096 bins over one zone, a range of 1e-3 of the domain): the bounds above lean on a row holding
many points - an interpolated v_q of D1D^dim random dofs can be far smaller than sum |B| |v_d|, and its rounding error is
relative to the latter; over many points that averages out, in a row of one point it shows (3D Q5Q4 under 4096 bins: 820 eps
of |m v_q| at a point whose v_y nearly cancels).  There `abs` is formed with every interpolated factor replaced by its
interpolation of absolute values (profile_ref's `cond`, >= abs): the condition of the interpolation itself.
Sums of the rows against lgh_diagnostics: the global sum bound of test_gpu_diagnostics (NQ + c and NE + c terms).
Everything "same bits" compares the raw bytes of the (nbins + 2) x 10 table."""
import os
import threading

import numpy as np
import pytest

import profile_cases as pc
import profile_ref as pr

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
BIG = [("1D-257", (3, 2)), ("2D-3x2", (4, 3)), ("3D-5x5x3", (3, 2)), ("3D-2x2x1", (5, 4))]


@pytest.fixture(scope="module")
def cases():
    from test_gpu_diagnostics import Case
    made = {}

    def get(zones_id, order):
        key = (zones_id, order)
        if key not in made:
            c = Case(pc.ZONES[zones_id], order[0], order[1]).setup()
            c.data = pc.case_data(pc.ZONES[zones_id], *order)
            assert np.array_equal(c.S, c.data["S"]) and np.array_equal(c.rho0_q, c.data["rho0_q"])   # the states the CPU test looked at
            c.refs = {}
            made[key] = c
        return made[key]
    yield get
    for c in made.values():
        c.close()


def run(c, spec, Sd=None, raw=False):
    _, axis, nbins, lo, hi, origin = spec
    p = c.ctx.profile(c.Sd if Sd is None else Sd, axis, nbins, lo, hi, origin)
    return p if not raw else p["rows"].copy().view(np.uint64)


def reference(c, spec, S=None):
    if S is not None:
        return pc.reference(c.data, spec, S=S, m=c.m)
    if spec not in c.refs:
        c.refs[spec] = pc.reference(c.data, spec, m=c.m)
    return c.refs[spec]


def check_rows(dim, ND, got, n_excl, ref, what="", rows=None, skip=(), few=False):
    """the bounds of the module docstring, for the rows given (default: all); few: rows of a handful of points (see there)"""
    assert not np.isnan(got).any() or skip, (what, "an entry was not written")
    R = ref["rows"].shape[0]
    rows = range(R) if rows is None else rows
    want, ab, kappa = ref["rows"], ref["cond" if few else "abs"], ref["kappa"]
    c = dim * ND + 8
    factor = {1: c * max(1.0, kappa), 2: 1.0, 3: c, 4: c, 5: c, 6: c * max(1.0, kappa), 7: c}
    assert n_excl == ref["n_excluded"], (what, n_excl, ref["n_excluded"])
    tol = max(1e-13, 2.0 * EPS * kappa)
    for r in rows:
        assert got[r, 0] == want[r, 0], (what, r, "n", got[r, 0], want[r, 0])
        for k in pr.SUM_COLS:
            if (r, k) in skip:
                continue
            bound = factor[k] * EPS * ab[r, k] + (EPS * ref["mom_extra"][r] if k == 5 else 0.0)
            err = abs(got[r, k] - want[r, k])
            assert err <= bound, (what, r, pr.COLS[k], got[r, k], want[r, k], err, bound)
        for k in (8, 9):
            if np.isfinite(want[r, k]):
                assert abs(got[r, k] - want[r, k]) <= tol * abs(want[r, k]), (what, r, pr.COLS[k])
            else:
                assert got[r, k] == want[r, k], (what, r, pr.COLS[k])
    worst = max((abs(got[r, k] - want[r, k]) / (EPS * ab[r, k]) for r in rows for k in pr.SUM_COLS if ab[r, k] > 0 and (r, k) not in skip and np.isfinite(ab[r, k])),
                default=0.0)
    print(f"{what}: largest error {worst:.2f} x 2^-52 sum|addend|")


@pytest.mark.parametrize("zones_id,order", pc.CASES, ids=pc.IDS)
def test_rows_match_numpy(cases, zones_id, order):
    c = cases(zones_id, order)
    for spec in pc.specs(c.dim):
        ref = reference(c, spec)
        assert pr.undecided(ref) == 0
        p = run(c, spec)
        check_rows(c.dim, c.ND, p["rows"], p["n_excluded"], ref, f"{zones_id} Q{order[0]}Q{order[1]} {spec[0]}")
        assert p["rows"].shape == (spec[2] + 2, 10) and np.array_equal(p["edges"], spec[3] + (spec[4] - spec[3]) * np.arange(spec[2] + 1) / spec[2])
        inner = p["rows"][1:-1]
        full = inner[:, 2] != 0
        assert np.array_equal(p["rho"][full], inner[full, 2] / inner[full, 1]) and np.isnan(p["rho"][~full]).all()
        assert np.array_equal(p["xi"][full], inner[full, 7] / inner[full, 2]) and np.array_equal(p["v"][full], inner[full, 5] / inner[full, 2])
        assert np.array_equal(p["e"][full], inner[full, 3] / inner[full, 2]) and np.array_equal(p["p"][full], inner[full, 6] / inner[full, 1])


@pytest.mark.parametrize("zones_id,order", pc.CASES, ids=pc.IDS)
def test_rows_add_up_to_the_diagnostics(cases, zones_id, order):
    c = cases(zones_id, order)
    g = c.glob()
    for spec in pc.specs(c.dim)[:1] + pc.specs(c.dim)[-1:]:
        ref, p = reference(c, spec), run(c, spec)
        rows = p["rows"]
        assert rows[:, 0].sum() + p["n_excluded"] == c.NE * c.NQ
        if p["n_excluded"] == 0:      # (lgh_diagnostics sums over every point, the profile leaves the inverted ones out)
            for slot, col in ((0, 2), (1, 1), (2, 3), (3, 4)):
                bound = (c.sum_bound(c.NQ) + c.sum_bound(c.NE)) * ref["abs"][:, col].sum()
                assert abs(rows[:, col].sum() - g[slot]) <= bound, (spec[0], pr.COLS[col], rows[:, col].sum(), g[slot], bound)


@pytest.mark.parametrize("zones_id,order", BIG)
def test_same_bits_every_time_and_on_both_atomic_paths(cases, zones_id, order, monkeypatch):
    """repeated calls, and LGH_PROFILE_FOLD = 0 (every lane sends its own atomics), 1, the default 8 and 100000 (every wavefront
    folds its lanes row by row, whatever the range): the same bytes.  A context's switches are those of the environment at its
    creation, so every other value gets a context of its own on the same data."""
    from test_gpu_diagnostics import Case
    c = cases(zones_id, order)
    specs = pc.specs(c.dim)[:1] + pc.specs(c.dim)[-2:]
    first = [run(c, spec, raw=True) for spec in specs]
    for spec, want in zip(specs, first):
        assert np.array_equal(want, run(c, spec, raw=True))
    for fold in ("0", "1", "100000"):
        monkeypatch.setenv("LGH_PROFILE_FOLD", fold)
        other = Case(pc.ZONES[zones_id], order[0], order[1]).setup()
        try:
            assert np.array_equal(other.S, c.S)
            for spec, want in zip(specs, first):
                assert np.array_equal(want, run(other, spec, raw=True)), (spec[0], fold)
        finally:
            other.close()
    monkeypatch.delenv("LGH_PROFILE_FOLD")
    for spec, want in zip(specs, first):
        assert np.array_equal(want, run(c, spec, raw=True))


@pytest.mark.parametrize("renumber", ["random", "mfem"])
def test_same_bits_under_every_numbering(renumber):
    """3 x 2 x 2 zones, Q3Q2, under another numbering of nodes and zones (the Case of
    test_gpu_diagnostics.test_outputs_sit_at_the_callers_zone_ids) and the same data - tables included - in the generator's
    lexicographic numbering: the same bytes"""
    from laghos_amd import host_lib
    from laghos_amd.context import Context
    from test_gpu_diagnostics import Case
    c = Case(pc.ZONES["3D-3x2x2"], 3, 2, renumber).setup()
    lex = None
    try:
        assert not np.array_equal(c.node_perm, np.arange(c.N))
        if renumber == "random":
            assert not np.array_equal(c.elem_perm, np.arange(c.NE))
        # zone j is the structured zone elem_perm[j], structured node i is node node_perm[i]
        inv = np.argsort(c.elem_perm)
        inv_node = np.argsort(c.node_perm)
        nodes = lambda a, ncomp: np.concatenate([a[k * c.N:(k + 1) * c.N][c.node_perm] for k in range(ncomp)])
        zones = lambda a, per: a.reshape(c.NE, per)[inv].reshape(-1)
        H1V, NL = 3 * c.N, c.L ** 3
        S_lex = np.concatenate([nodes(c.S[:2 * H1V], 6), zones(c.S[2 * H1V:], NL)])
        h1map_lex = np.ascontiguousarray(inv_node[c.h1map.reshape(c.NE, c.ND)[inv]].astype(np.int32).reshape(-1))
        ess = host_lib.host_disc("cartesian", 0, 3, 2, 1, zones=pc.ZONES["3D-3x2x2"], renumber=renumber, seed=5)["ess"]
        ess_lex = [np.sort(inv_node[np.asarray(e, dtype=np.int64)]).astype(np.int32) for e in ess]
        lex = Context(3, c.NE, c.D, c.Q, c.L, c.N, h1map_lex, c.B, c.G, c.Bl, c.W, c.gamma[inv], ess_lex, order_v=3)
        lex.setup_rho0detj0(lex.to_dev(nodes(c.x0, 3)), lex.to_dev(zones(c.rho0_l2, NL)), lex.to_dev(zones(c.rho0_q, c.NQ)))
        # the masses of the points are inputs here, not what is tested: the lexicographic context gets the very masses of the renumbered one
        assert np.allclose(lex.rho0DetJ0w, zones(c.m, c.NQ), rtol=1e-13, atol=0.0)
        lex._write(lex.lib.lgh_qdata_rho0DetJ0w(lex.h), zones(c.m, c.NQ))
        assert np.array_equal(lex.rho0DetJ0w, zones(c.m, c.NQ))
        Sd_lex = lex.to_dev(S_lex)
        for spec in pc.specs(3):
            _, axis, nbins, lo, hi, origin = spec
            a, b = run(c, spec), lex.profile(Sd_lex, axis, nbins, lo, hi, origin)
            assert a["rows"][:, 0].sum() + a["n_excluded"] == c.NE * c.NQ and a["rows"][1:-1, 2].sum() > 0
            assert np.array_equal(a["rows"].view(np.uint64), b["rows"].view(np.uint64)), spec[0]
            assert a["n_excluded"] == b["n_excluded"]
    finally:
        c.close()
        if lex is not None:
            lex.close()


def test_two_emulated_ranks():
    """3D, 4 x 2 x 2 zones on two ranks: see _two_emulated_ranks"""
    _two_emulated_ranks(["-dim", 3, "-nx", 4, "-ny", 2, "-nz", 2, "-Sx", 2, "-Sy", 1, "-Sz", 1],
                        [("x", 5, 0.0, 2.0, None), ("r", 6, 0.0, 2.5, (0.0, 0.0, 0.0)), ("z", 3, 0.1, 0.9, None)])


def test_two_emulated_ranks_2d():
    """the same on 2D blocks: 4 x 2 zones on two ranks, binned along x, r and y"""
    _two_emulated_ranks(["-dim", 2, "-nx", 4, "-ny", 2, "-Sx", 2, "-Sy", 1],
                        [("x", 5, 0.0, 2.0, None), ("r", 6, 0.0, 2.5, (0.0, 0.0)), ("y", 3, 0.1, 0.9, None)])


def _two_emulated_ranks(mesh_args, looks):
    """3D, 4 x 2 x 2 zones, Q2Q1 on two ranks (threads, "LGHLOCAL" communicator; the harness of
    test_gpu_diagnostics.test_two_emulated_ranks).  At the initial state (the same bits on every partition) both ranks return
    the bytes of the one-rank run; after two steps (the states of a one-rank run differ by then, in the last bits of the CG
    sums) both ranks still return the same bytes, with values of their own in every column."""
    from laghos_amd import host_lib
    args = mesh_args + ["-rs", 0, "-p", 1, "-ok", 2, "-ot", 1, "-pa", "-tf", 1e9, "-ms", 10 ** 6, "-vs", 10 ** 9, "-q"]

    def run_rank(nranks, rank, cid, out, err):
        try:
            sim = host_lib.Sim(args, nranks=nranks, rank=rank, nccl_id=cid)
            sim.enable_timers(False)
            first = [sim.profile(*l) for l in looks]
            for _ in range(2):
                assert sim.step() == 1
            out[rank] = (first, [sim.profile(*l) for l in looks], sim.sizes())
            sim.close()
        except Exception as ex:  # noqa: BLE001 - reported below
            err[rank] = repr(ex)

    one, err = {}, {}
    run_rank(1, 0, None, one, err)
    assert not err, err
    cid = (b"LGHLOCAL" + os.urandom(16).hex().encode()).ljust(128, b"\0")
    two = {}
    th = [threading.Thread(target=run_rank, args=(2, r, cid, two, err), daemon=True) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in th) and not err, err
    npts = one[0][2]["global_NE"] * one[0][2]["NQ"]
    for k in range(len(looks)):
        ref, a, b = one[0][0][k], two[0][0][k], two[1][0][k]
        assert not np.isnan(ref["rows"]).any() and ref["rows"][:, 0].sum() == npts and ref["n_excluded"] == 0
        assert ref["rows"][:, 2].sum() > 0 and ref["rows"][:, 3].sum() > 0
        assert np.array_equal(a["rows"].view(np.uint64), ref["rows"].view(np.uint64)), looks[k]
        assert np.array_equal(b["rows"].view(np.uint64), ref["rows"].view(np.uint64)), looks[k]
        assert a["n_excluded"] == b["n_excluded"] == 0
        a, b = two[0][1][k], two[1][1][k]
        assert not np.isnan(a["rows"]).any() and np.array_equal(a["rows"].view(np.uint64), b["rows"].view(np.uint64)), looks[k]
        assert a["rows"][:, 0].sum() == npts and a["rows"][:, 4].sum() > 0 and np.abs(a["rows"][:, 5]).sum() > 0


def domain_spec(name, axis, nbins, lo, hi, origin=None):
    return (name, axis, nbins, lo, hi, origin)


def test_one_bin(cases):
    c = cases("3D-3x2x2", (2, 1))
    spec = domain_spec("one", 0, 1, -1.0, 2.0)
    ref, p = reference(c, spec), run(c, spec)
    assert pr.undecided(ref) == 0 and p["rows"][1, 0] + p["n_excluded"] == c.NE * c.NQ
    check_rows(c.dim, c.ND, p["rows"], p["n_excluded"], ref, "one bin")


def test_4096_bins_over_one_zone(cases):
    """one zone of Q3Q2 (64 points) under 4096 bins: the wide-range path; every row holds 0 or a few points and an empty row
    is 0 ... +inf -inf"""
    c = cases("1D-1", (3, 2))
    c3 = cases("3D-2x2x1", (5, 4))
    for cc, spec in ((c, domain_spec("4096", 0, 4096, 0.0, 1.0)), (c3, domain_spec("4096-3d", 1, 4096, 0.0, 1.0)),
                     (c3, domain_spec("4096-r", 3, 4096, 0.0, 1.8, (0.0, 0.0, 0.0)))):
        ref, p = reference(cc, spec), run(cc, spec)
        assert pr.undecided(ref) == 0
        rows = p["rows"]
        check_rows(cc.dim, cc.ND, rows, p["n_excluded"], ref, spec[0], few=True)
        empty = rows[:, 0] == 0
        assert empty.sum() >= 4096 + 2 - cc.NE * cc.NQ and rows[:, 0].max() <= 64
        assert np.all(rows[empty, :8] == 0) and np.all(np.isposinf(rows[empty, 8])) and np.all(np.isneginf(rows[empty, 9]))


def test_ranges_beside_and_around_the_mesh(cases):
    c = cases("3D-5x5x3", (3, 2))
    npts = c.NE * c.NQ
    left = run(c, domain_spec("left", 0, 7, -3.0, -2.0))          # the range lies left of the mesh: everything is at or above hi
    assert left["rows"][-1, 0] + left["n_excluded"] == npts and np.all(left["rows"][:-1, :8] == 0)
    assert np.all(np.isposinf(left["rows"][:-1, 8])) and np.all(np.isneginf(left["rows"][:-1, 9]))
    right = run(c, domain_spec("right", 0, 7, 2.0, 3.0))          # ... right of it: everything is below lo
    assert right["rows"][0, 0] + right["n_excluded"] == npts and np.all(right["rows"][1:, :8] == 0)
    # the two outer rows hold the same points: exact sums give the same bits
    assert np.array_equal(left["rows"][-1, :5].view(np.uint64), right["rows"][0, :5].view(np.uint64))
    assert np.array_equal(left["rows"][-1, 6].view(np.uint64), right["rows"][0, 6].view(np.uint64))
    for spec in (domain_spec("one bin holds all", 0, 7, -4.5, 9.5), domain_spec("1e-3", 1, 7, 0.4, 0.401),
                 domain_spec("1e+3", 2, 7, -500.0, 500.0), domain_spec("r 1e+3", 3, 5, 0.0, 1000.0, (0.1, 0.2, 0.3))):
        ref, p = reference(c, spec), run(c, spec)
        assert pr.undecided(ref) == 0, spec[0]
        check_rows(c.dim, c.ND, p["rows"], p["n_excluded"], ref, spec[0], few=(spec[0] == "1e-3"))
    all_in_one = run(c, domain_spec("one bin holds all", 0, 7, -4.5, 9.5))["rows"]       # bin 2 is [-0.5, 1.5)
    assert all_in_one[3, 0] + left["n_excluded"] == npts and np.all(np.delete(all_in_one, 3, axis=0)[:, 0] == 0)   # maximal contention


BREAKS3 = [[0, .3, .7, 1], [0, .5, 1], [0, .4, 1]]          # 12 zones (test_gpu_diagnostics)


@pytest.fixture(scope="module")
def edge():
    from helpers import make_gpu
    from oracle.fem import Problem
    prob = Problem(breaks=BREAKS3, order_v=2, order_e=1, problem=1)
    g = make_gpu(prob)
    m = g.ctx.rho0DetJ0w

    def look(S, spec):
        _, axis, nbins, lo, hi, origin = spec
        p = g.profile(g.ctx.to_dev(S), axis, nbins, lo, hi, origin)
        ref = pr.profile_reference(3, prob.NE, prob.N, prob.D1D, prob.L1D, np.asarray(prob.h1map).reshape(-1), S, m, prob.initial_state()[2],
                                   prob.W, prob.B, prob.G, prob.Bl, axis, nbins, lo, hi, origin)
        return p, ref
    yield prob, look
    g.close()


def test_edge_inverted_layer(edge):
    import edge_states as es
    prob, look = edge
    for spec in (domain_spec("x", 0, 6, 0.0, 1.0), domain_spec("r", 3, 5, 0.0, 1.8, (0.0, 0.0, 0.0))):
        p, ref = look(es.edge_state(prob, "inverted_layer"), spec)
        assert pr.undecided(ref) == 0
        assert ref["n_excluded"] > 0 and ref["n_excluded"] % prob.NQ == 0          # whole zones: the reflected layer
        check_rows(3, prob.ND, p["rows"], p["n_excluded"], ref, "inverted layer " + spec[0])
        assert p["rows"][:, 0].sum() == prob.NE * prob.NQ - ref["n_excluded"]
        assert np.all(p["rows"][:, 1] >= 0) and np.all(p["rows"][p["rows"][:, 0] > 0, 8] > 0)   # no negative volume, no negative density


def test_edge_all_negative_e(edge):
    import edge_states as es
    prob, look = edge
    p, ref = look(es.edge_state(prob, "all_negative_e"), domain_spec("y", 1, 4, 0.0, 1.0))
    check_rows(3, prob.ND, p["rows"], p["n_excluded"], ref, "all negative e")
    assert np.all(p["rows"][:, 6] == 0.0) and np.all(p["rows"][1:-1, 3] < 0) and p["n_excluded"] == 0


def test_a_nan_coordinate_stays_in_its_zones(cases):
    """one x coordinate of one node of 3 x 2 x 2 zones is NaN: the points of the zones that hold the node are excluded, and
    nothing else - every column of every row stays finite and is the reference's"""
    c = cases("3D-3x2x2", (2, 1))
    hm = c.h1map.reshape(c.NE, c.ND)
    node = hm[5, 0]                                     # a corner of zone 5: shared
    holders = np.nonzero((hm == node).any(axis=1))[0]
    assert 1 < len(holders) < c.NE
    S = c.S.copy()
    S[c.N + node] = np.nan                              # its y coordinate
    Sd = c.ctx.to_dev(S)
    for spec in pc.specs(3)[:1] + pc.specs(3)[-2:]:
        p = run(c, spec, Sd)
        ref = reference(c, spec, S)
        assert p["n_excluded"] == len(holders) * c.NQ + reference(c, spec)["n_excluded"]
        inner = p["rows"][:, :8]
        assert np.isfinite(inner).all()
        check_rows(c.dim, c.ND, p["rows"], p["n_excluded"], ref, "NaN coordinate " + spec[0])


def test_an_overflowing_addend_poisons_its_entry_only(cases):
    """the interior node of one Q2Q1 zone moves at 1e200: m |v|^2 overflows at every point of that zone (finite factors); the ke
    of the rows that hold such a point is NaN, their other columns are the reference's, and the next call on the clean state is
    clean"""
    c = cases("3D-3x2x2", (2, 1))
    spec = pc.specs(3)[0]
    clean = run(c, spec, raw=True)
    hm = c.h1map.reshape(c.NE, c.ND)
    node = hm[5, 13]                                    # the middle node of 3 x 3 x 3
    assert (hm == node).sum() == 1
    S = c.S.copy()
    for k in range(3):
        S[(3 + k) * c.N + node] = 1e200
    ref = reference(c, spec, S)
    bad = np.nonzero(np.isnan(ref["rows"][:, 4]))[0]
    assert 1 <= len(bad) < 7 and np.isfinite(ref["rows"][:, [1, 2, 3, 5, 6, 7]]).all()
    p = run(c, spec, c.ctx.to_dev(S))
    assert np.isnan(p["rows"][bad, 4]).all() and np.isnan(p["rows"]).sum() == len(bad)
    check_rows(c.dim, c.ND, p["rows"], p["n_excluded"], ref, "overflow", rows=bad, skip={(r, 4) for r in bad})
    assert np.array_equal(clean, run(c, spec, raw=True))


def test_quiet_mesh_around_one_loud_zone(cases):
    """e and v scaled by 1e-12 everywhere but in one zone (the idea of test_gpu_k1's quiet-mesh case): ke addends of the quiet
    rows are 2^-80 of the largest; every row still meets the bounds relative to its own sum |addend|"""
    c = cases("3D-5x5x3", (3, 2))
    hm = c.h1map.reshape(c.NE, c.ND)
    loud = 37
    S = c.S.copy()
    H1V, NL = 3 * c.N, c.L ** 3
    quiet_nodes = np.setdiff1d(np.arange(c.N), hm[loud])
    for k in range(3):
        S[H1V + k * c.N + quiet_nodes] *= 1e-12
    e = S[2 * H1V:].reshape(c.NE, NL)
    e[np.arange(c.NE) != loud] *= 1e-12
    Sd = c.ctx.to_dev(S)
    for spec in pc.specs(3)[:1] + pc.specs(3)[-2:]:
        ref, p = reference(c, spec, S), run(c, spec, Sd)
        assert pr.undecided(ref) == 0
        ke = ref["abs"][1:-1, 4]
        # quiet rows exist: along x whole bins lie away from the loud zone (addends 1e-24 of the largest); a shell around a
        # point outside the mesh always cuts zones that share a loud node, whose quiet side still is 1e-9 of the loud one
        assert ke[ke > 0].min() < (1e-20 if spec[1] == 0 else 1e-9) * ke.max(), spec[0]
        check_rows(c.dim, c.ND, p["rows"], p["n_excluded"], ref, "quiet mesh " + spec[0])


def test_nothing_else_moves():
    """a profile taken between two steps must not change the next step (test_gpu_diagnostics.test_nothing_else_moves)"""
    from helpers import deformed_state, make_gpu
    from oracle.fem import Problem
    prob = Problem(mesh="cube01_hex", rs=1, order_v=3, order_e=2, problem=1)
    g = make_gpu(prob)
    try:
        ctx = g.ctx
        S = deformed_state(prob, seed=5)
        Sd = ctx.to_dev(S)
        ctx.set_dt_est(float("inf"))
        ctx.qupdate(Sd)
        ctx.sync()

        def products():
            f1, ftv = ctx.zeros(prob.H1V), ctx.zeros(prob.L2V)
            assert ctx.fused_force_mult(f1) and ctx.fused_force_mult_transpose(ftv)
            ctx.sync()
            return f1.cpu().numpy(), ftv.cpu().numpy()

        before = products()
        gen, dt = ctx.quadrature_generation(), ctx.get_dt_est()
        assert gen[1] == 1 and gen[2] == 1 and np.isfinite(dt)
        p = ctx.profile(Sd, "r", 16, 0.0, 2.0, (0.0, 0.0, 0.0))
        q = g.profile(Sd, "x", 4096, 0.0, 1.0)
        assert p["rows"][:, 2].sum() > 0 and q["rows"][:, 0].sum() == prob.NE * prob.NQ
        assert ctx.quadrature_generation() == gen and ctx.get_dt_est() == dt
        assert np.array_equal(Sd.cpu().numpy(), S)
        after = products()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    finally:
        g.close()


def test_refusals():
    """LGH_ERR_ARG (error 1) and no launch: before the set-up, and for every bad spec"""
    from laghos_amd._lib import LghError
    from test_gpu_diagnostics import Case
    c = Case(pc.ZONES["2D-3x2"], 2, 1)
    try:
        Sd = c.ctx.to_dev(c.S)
        with pytest.raises(LghError, match="error 1: .*lgh_setup_rho0detj0"):
            c.ctx.profile(Sd, 0, 7, 0.0, 1.0)
        c.setup()
        good = c.ctx.profile(c.Sd, 0, 7, 0.0, 1.0)
        assert good["rows"][:, 0].sum() + good["n_excluded"] == c.NE * c.NQ
        inf, nan = float("inf"), float("nan")
        bad = [(2, 7, 0.0, 1.0, None), ("z", 7, 0.0, 1.0, None), (4, 7, 0.0, 1.0, None), (-1, 7, 0.0, 1.0, None),
               (0, 0, 0.0, 1.0, None), (0, 4097, 0.0, 1.0, None), (0, -3, 0.0, 1.0, None),
               (0, 7, 1.0, 1.0, None), (0, 7, 2.0, 1.0, None), (0, 7, nan, 1.0, None), (0, 7, 0.0, inf, None), (0, 7, -inf, 0.0, None),
               (3, 7, 0.0, 1.0, (nan, 0.0)), (3, 7, 0.0, 1.0, (0.0, inf))]
        for axis, nbins, lo, hi, origin in bad:
            with pytest.raises(LghError, match="error 1: "):
                c.ctx.profile(c.Sd, axis, nbins, lo, hi, origin)
        # a non-finite third origin component is ignored in 2D, and an origin is ignored for an axis
        assert np.array_equal(c.ctx.profile(c.Sd, 3, 7, 0.0, 1.0, (0.0, 0.0, nan))["rows"].view(np.uint64),
                              c.ctx.profile(c.Sd, 3, 7, 0.0, 1.0, (0.0, 0.0, 5.0))["rows"].view(np.uint64))
        assert np.array_equal(c.ctx.profile(c.Sd, 0, 7, 0.0, 1.0, (nan, nan, nan))["rows"].view(np.uint64), good["rows"].view(np.uint64))
        import ctypes
        from laghos_amd import _lib
        L = _lib.load()
        spec = _lib.LghProfileSpec(0, 7, 0.0, 1.0)
        out, n = np.zeros(90), ctypes.c_long(0)
        dp = out.ctypes.data_as(_lib.c_dbl_p)
        S_ptr = ctypes.c_void_p(c.Sd.data_ptr())
        for call in (lambda: L.lgh_profile(c.ctx.h, None, ctypes.byref(spec), dp, ctypes.byref(n)),
                     lambda: L.lgh_profile(c.ctx.h, S_ptr, None, dp, ctypes.byref(n)),
                     lambda: L.lgh_profile(c.ctx.h, S_ptr, ctypes.byref(spec), None, ctypes.byref(n)),
                     lambda: L.lgh_profile(c.ctx.h, S_ptr, ctypes.byref(spec), dp, None),
                     lambda: L.lgh_profile(None, S_ptr, ctypes.byref(spec), dp, ctypes.byref(n))):
            assert call() == 1
        assert not out.any()
    finally:
        c.close()
