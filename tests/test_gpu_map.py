"""lgh_map (Context.map, Sim.map): the flow binned onto a fixed Cartesian grid with exact, order-free cell sums, against the
numpy restatement of tests/map_ref.py, the figures of lgh_diagnostics, lgh_profile where a map is a profile, and the edge
states of tests/edge_states.py.  The file mirrors tests/test_gpu_profile.py.

States are those of tests/test_gpu_diagnostics.py (its `Case`; tests/map_cases.py names the grids, and tests/test_map_ref.py
holds every (case, grid) to `undecided == 0` on the CPU: no point within 1e-9 of a cell edge or of detJ = 0 - which is what
lets the counts be demanded exactly here).

Bounds per row, those of tests/test_gpu_profile.py (none taken from what the kernel gives); abs = sum |addend| of the row's
points, c = dim D1D^dim + 8:
  n                  exact;
  rho_min, rho_max   relative max(1e-13, 2 eps kappa);
  ie, ke, mom_c      c 2^-52 abs (every momentum column takes the bound of ie);
  mass               2^-52 abs;
  vol, pv            c max(1, kappa) 2^-52 abs.
A cell holds far fewer points than a bin of a profile, and the bounds above lean on a row holding many (the docstring there:
an interpolated v_q can be far smaller than sum |B| |v_d|, to which its rounding error is relative; over many points that
averages out, in a row of a few it shows).  So a row of fewer than 8 points - the "handful" of that file, decided by the
reference's count, never by what the kernel returns - takes `cond` for `abs`, as the 4096-bin rows do there.
Sums of the rows against lgh_diagnostics: the global sum bound of test_gpu_diagnostics (NQ + c and NE + c terms).
Everything "same bits" compares the raw bytes of the (ncells + 1) x 11 table."""
import os
import threading

import numpy as np
import pytest

import map_cases as mc
import map_ref as mr

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
FEW = 8
BIG = [("1D-257", (3, 2)), ("2D-3x2", (4, 3)), ("3D-5x5x3", (3, 2)), ("3D-2x2x1", (5, 4))]


@pytest.fixture(scope="module")
def cases():
    from test_gpu_diagnostics import Case
    made = {}

    def get(zones_id, order):
        key = (zones_id, order)
        if key not in made:
            c = Case(mc.ZONES[zones_id], order[0], order[1]).setup()
            c.data = mc.case_data(mc.ZONES[zones_id], *order)
            assert np.array_equal(c.S, c.data["S"]) and np.array_equal(c.rho0_q, c.data["rho0_q"])   # the states the CPU test looked at
            c.points, c.refs = None, {}
            made[key] = c
        return made[key]
    yield get
    for c in made.values():
        c.close()


def run(c, g, Sd=None, raw=False):
    p = c.ctx.map(c.Sd if Sd is None else Sd, g[1], g[2], g[3])
    return p if not raw else p["rows"].copy().view(np.uint64)


def reference(c, g, S=None):
    """the reference of a case under a grid; the points of the case's own state are evaluated once and shared"""
    if S is not None:
        return mc.reference(mc.points(c.data, S=S, m=c.m), g)
    if c.points is None:
        c.points = mc.points(c.data, m=c.m)
    if g not in c.refs:
        c.refs[g] = mc.reference(c.points, g)
    return c.refs[g]


def check_rows(dim, ND, got, n_excl, ref, what="", rows=None, skip=()):
    """the bounds of the module docstring, for the rows given (default: all)"""
    want, kappa = ref["rows"], ref["kappa"]
    assert got.shape == want.shape, (what, got.shape, want.shape)
    rows = list(range(want.shape[0]) if rows is None else rows)
    assert not np.isnan(got[rows]).any() or skip, (what, "an entry was not written")
    c = dim * ND + 8
    factor = {1: c * max(1.0, kappa), 2: 1.0, 3: c, 4: c, 5: c, 6: c, 7: c, 8: c * max(1.0, kappa)}
    assert n_excl == ref["n_excluded"], (what, n_excl, ref["n_excluded"])
    tol = max(1e-13, 2.0 * EPS * kappa)
    worst = 0.0
    for r in rows:
        assert got[r, 0] == want[r, 0], (what, r, "n", got[r, 0], want[r, 0])
        ab = ref["cond" if want[r, 0] < FEW else "abs"][r]
        for k in mr.SUM_COLS:
            if (r, k) in skip:
                continue
            bound = factor[k] * EPS * ab[k]
            err = abs(got[r, k] - want[r, k])
            assert err <= bound, (what, r, mr.COLS[k], got[r, k], want[r, k], err, bound)
            if ab[k] > 0 and np.isfinite(ab[k]):
                worst = max(worst, err / (EPS * ab[k]))
        for k in (9, 10):
            if np.isfinite(want[r, k]):
                assert abs(got[r, k] - want[r, k]) <= tol * abs(want[r, k]), (what, r, mr.COLS[k])
            else:
                assert got[r, k] == want[r, k], (what, r, mr.COLS[k])
    print(f"{what}: largest error {worst:.2f} x 2^-52 sum|addend|")


def check_dict(p, dim, g):
    """shape of grid, edges and the derived arrays"""
    n = list(g[1]) + [1] * (3 - dim)
    nc = n[0] * n[1] * n[2]
    rows = p["rows"]
    assert rows.shape == (nc + 1, 11) and p["grid"].shape == (n[2], n[1], n[0], 11)
    assert np.array_equal(p["outside"].view(np.uint64), rows[0].view(np.uint64))
    assert np.array_equal(p["grid"].reshape(nc, 11).view(np.uint64), rows[1:].view(np.uint64))
    assert len(p["edges"]) == dim
    for a in range(dim):
        assert np.array_equal(p["edges"][a], g[2][a] + (g[3][a] - g[2][a]) * np.arange(n[a] + 1) / n[a])
    cell = rows[1:]
    full, vol = cell[:, 2] != 0, cell[:, 1] != 0
    assert p["rho"].shape == p["e"].shape == p["p"].shape == (n[2], n[1], n[0]) and p["v"].shape == (n[2], n[1], n[0], dim)
    flat = lambda a: a.reshape(nc, -1) if a.ndim == 4 else a.reshape(nc)
    assert np.array_equal(flat(p["rho"])[vol], cell[vol, 2] / cell[vol, 1]) and np.isnan(flat(p["rho"])[~vol]).all()
    assert np.array_equal(flat(p["p"])[vol], cell[vol, 8] / cell[vol, 1]) and np.isnan(flat(p["p"])[~vol]).all()
    assert np.array_equal(flat(p["e"])[full], cell[full, 3] / cell[full, 2]) and np.isnan(flat(p["e"])[~full]).all()
    assert np.array_equal(flat(p["v"])[full], cell[full, 5:5 + dim] / cell[full, 2:3]) and np.isnan(flat(p["v"])[~full]).all()
    # a momentum component above the dimension is exactly +0.0
    assert np.all(rows[:, 5 + dim:8].view(np.uint64) == 0)
    empty = rows[:, 0] == 0
    assert np.all(rows[empty, :9] == 0) and np.all(np.isposinf(rows[empty, 9])) and np.all(np.isneginf(rows[empty, 10]))


@pytest.mark.parametrize("zones_id,order", mc.CASES, ids=mc.IDS)
def test_rows_match_numpy(cases, zones_id, order):
    c = cases(zones_id, order)
    for g in mc.grids(c.dim):
        ref = reference(c, g)
        assert mr.undecided(ref) == 0
        p = run(c, g)
        check_rows(c.dim, c.ND, p["rows"], p["n_excluded"], ref, f"{zones_id} Q{order[0]}Q{order[1]} {g[0]}")
        check_dict(p, c.dim, g)


@pytest.mark.parametrize("zones_id,order", mc.CASES, ids=mc.IDS)
def test_rows_add_up_to_the_diagnostics(cases, zones_id, order):
    c = cases(zones_id, order)
    glob = c.glob()
    for g in mc.grids(c.dim):
        ref, p = reference(c, g), run(c, g)
        rows = p["rows"]
        assert rows[:, 0].sum() + p["n_excluded"] == c.NE * c.NQ
        if p["n_excluded"] == 0:      # (lgh_diagnostics sums over every point, the map leaves the inverted ones out)
            for slot, col in ((0, 2), (1, 1), (2, 3), (3, 4)):
                bound = (c.sum_bound(c.NQ) + c.sum_bound(c.NE)) * ref["abs"][:, col].sum()
                assert abs(rows[:, col].sum() - glob[slot]) <= bound, (g[0], mr.COLS[col], rows[:, col].sum(), glob[slot], bound)


def test_excluded_points_are_covered(cases):
    for zones_id, order in (("3D-5x5x3", (3, 2)), ("3D-2x2x1", (5, 4))):
        c = cases(zones_id, order)
        p = run(c, mc.grid("unit", 3))
        assert p["n_excluded"] > 0 and p["n_excluded"] == reference(c, mc.grid("unit", 3))["n_excluded"]


@pytest.mark.parametrize("zones_id,order", mc.CASES, ids=mc.IDS)
def test_the_slab_is_the_profile_along_x(cases, zones_id, order):
    """(9, 1, 1) cells against lgh_profile along x with 9 bins over [0, 1]: n equal exactly, every common sum column within the
    sum of the bounds each has against numpy (not bit for bit: the two kernels may round an addend differently).  Under
    `slab-wide` (one cell across y and z that holds every point) all inner rows are compared; under `slab` itself, whose box
    ends at y, z = 0 and 1 where the curved boundary crosses, the rows that lose no point there - by the references' counts."""
    import profile_cases as pc
    import profile_ref as pr
    c = cases(zones_id, order)
    spec = ("x", 0, 9, 0.0, 1.0, None)
    pref = pc.reference(c.data, spec, m=c.m)
    assert pr.undecided(pref) == 0
    prof = c.ctx.profile(c.Sd, 0, 9, 0.0, 1.0)["rows"][1:-1]
    cc = c.dim * c.ND + 8
    kap = max(1.0, pref["kappa"])
    factor = dict(zip(mc.PROFILE_COLS[1:7], (cc * kap, 1.0, cc, cc, cc, cc * kap)))     # vol mass ie ke mom pv: test_gpu_profile
    for g in (mc.slab_wide(c.dim), mc.grid("slab", c.dim)):
        ref = reference(c, g)
        assert mr.undecided(ref) == 0
        got = run(c, g)["rows"][1:]
        same = ref["rows"][1:, 0] == pref["rows"][1:-1, 0]
        assert same.all() or (g[0] == "slab" and c.dim > 1)
        for r in np.nonzero(same)[0]:
            assert got[r, 0] == prof[r, 0], (g[0], r)
            few = pref["rows"][1 + r, 0] < FEW
            for km, kp in zip(mc.SLAB_COLS[1:7], mc.PROFILE_COLS[1:7]):
                bound = factor[kp] * EPS * (ref["cond" if few else "abs"][1 + r, km] + pref["cond" if few else "abs"][1 + r, kp])
                assert abs(got[r, km] - prof[r, kp]) <= bound, (g[0], r, mr.COLS[km], got[r, km], prof[r, kp], bound)
            for km, kp in ((9, 8), (10, 9)):                                     # each within its bound against numpy
                if np.isfinite(prof[r, kp]):
                    assert abs(got[r, km] - prof[r, kp]) <= 2 * max(1e-13, 2.0 * EPS * pref["kappa"]) * abs(prof[r, kp])
                else:
                    assert got[r, km] == prof[r, kp]                           # an empty row: +inf, -inf


@pytest.mark.parametrize("zones_id,order", BIG)
def test_same_bits_every_time_and_on_both_atomic_paths(cases, zones_id, order, monkeypatch):
    """repeated calls, and LGH_MAP_FOLD = 0 (every lane sends its own atomics), 1, the default 8 and 100000 (every wavefront
    folds all its cells): the same bytes, under `unit`, `fine` (every lane in a cell of its own) and `one` (every lane in one
    cell).  A context's switches are those of the environment at its creation, so every other value gets a context of its own."""
    from test_gpu_diagnostics import Case
    c = cases(zones_id, order)
    gs = [mc.grid(name, c.dim) for name in ("unit", "fine", "one")]
    first = [run(c, g, raw=True) for g in gs]
    for g, want in zip(gs, first):
        assert np.array_equal(want, run(c, g, raw=True))
    for fold in ("0", "1", "100000"):
        monkeypatch.setenv("LGH_MAP_FOLD", fold)
        other = Case(mc.ZONES[zones_id], order[0], order[1]).setup()
        try:
            assert np.array_equal(other.S, c.S)
            for g, want in zip(gs, first):
                assert np.array_equal(want, run(other, g, raw=True)), (g[0], fold)
        finally:
            other.close()
    monkeypatch.delenv("LGH_MAP_FOLD")
    for g, want in zip(gs, first):
        assert np.array_equal(want, run(c, g, raw=True))


@pytest.mark.parametrize("renumber", ["random", "mfem"])
def test_same_bits_under_every_numbering(renumber):
    """3 x 2 x 2 zones, Q3Q2, under another numbering of nodes and zones and the same data - tables included - in the
    generator's lexicographic numbering: the same bytes (the construction of tests/test_gpu_profile.py)"""
    from laghos_amd import host_lib
    from laghos_amd.context import Context
    from test_gpu_diagnostics import Case
    c = Case(mc.ZONES["3D-3x2x2"], 3, 2, renumber).setup()
    lex = None
    try:
        assert not np.array_equal(c.node_perm, np.arange(c.N))
        if renumber == "random":
            assert not np.array_equal(c.elem_perm, np.arange(c.NE))
        inv = np.argsort(c.elem_perm)
        inv_node = np.argsort(c.node_perm)
        nodes = lambda a, ncomp: np.concatenate([a[k * c.N:(k + 1) * c.N][c.node_perm] for k in range(ncomp)])
        zones = lambda a, per: a.reshape(c.NE, per)[inv].reshape(-1)
        H1V, NL = 3 * c.N, c.L ** 3
        S_lex = np.concatenate([nodes(c.S[:2 * H1V], 6), zones(c.S[2 * H1V:], NL)])
        h1map_lex = np.ascontiguousarray(inv_node[c.h1map.reshape(c.NE, c.ND)[inv]].astype(np.int32).reshape(-1))
        ess = host_lib.host_disc("cartesian", 0, 3, 2, 1, zones=mc.ZONES["3D-3x2x2"], renumber=renumber, seed=5)["ess"]
        ess_lex = [np.sort(inv_node[np.asarray(e, dtype=np.int64)]).astype(np.int32) for e in ess]
        lex = Context(3, c.NE, c.D, c.Q, c.L, c.N, h1map_lex, c.B, c.G, c.Bl, c.W, c.gamma[inv], ess_lex, order_v=3)
        lex.setup_rho0detj0(lex.to_dev(nodes(c.x0, 3)), lex.to_dev(zones(c.rho0_l2, NL)), lex.to_dev(zones(c.rho0_q, c.NQ)))
        # the masses of the points are inputs here, not what is tested: the lexicographic context gets the very masses of the renumbered one
        assert np.allclose(lex.rho0DetJ0w, zones(c.m, c.NQ), rtol=1e-13, atol=0.0)
        lex._write(lex.lib.lgh_qdata_rho0DetJ0w(lex.h), zones(c.m, c.NQ))
        assert np.array_equal(lex.rho0DetJ0w, zones(c.m, c.NQ))
        Sd_lex = lex.to_dev(S_lex)
        for g in mc.grids(3):
            a, b = run(c, g), lex.map(Sd_lex, g[1], g[2], g[3])
            assert a["rows"][:, 0].sum() + a["n_excluded"] == c.NE * c.NQ and a["rows"][1:, 2].sum() > 0
            assert np.array_equal(a["rows"].view(np.uint64), b["rows"].view(np.uint64)), g[0]
            assert a["n_excluded"] == b["n_excluded"]
    finally:
        c.close()
        if lex is not None:
            lex.close()


def test_two_emulated_ranks():
    """3D, 4 x 2 x 2 zones on two ranks, (5, 3, 2) cells over the domain: see _two_emulated_ranks"""
    _two_emulated_ranks(["-dim", 3, "-nx", 4, "-ny", 2, "-nz", 2, "-Sx", 2, "-Sy", 1, "-Sz", 1], ((5, 3, 2), (0.0, 0.0, 0.0), (2.0, 1.0, 1.0)))


def test_two_emulated_ranks_2d():
    """the same on 2D blocks: 4 x 2 zones on two ranks, (5, 3) cells over the domain"""
    _two_emulated_ranks(["-dim", 2, "-nx", 4, "-ny", 2, "-Sx", 2, "-Sy", 1], ((5, 3), (0.0, 0.0), (2.0, 1.0)))


def _two_emulated_ranks(mesh_args, look):
    """Q2Q1 on two ranks (threads, the in-process communicator; the harness of tests/test_gpu_profile.py).  At the initial state
    (the same bits on every partition) both ranks return the bytes of the one-rank run; after two steps (the states of a
    one-rank run differ by then, in the last bits of the CG sums) both ranks still return the same bytes, with values of their
    own in every column."""
    from laghos_amd import host_lib
    args = mesh_args + ["-rs", 0, "-p", 1, "-ok", 2, "-ot", 1, "-pa", "-tf", 1e9, "-ms", 10 ** 6, "-vs", 10 ** 9, "-q"]
    dim = len(look[0])

    def run_rank(nranks, rank, cid, out, err):
        try:
            sim = host_lib.Sim(args, nranks=nranks, rank=rank, nccl_id=cid)
            sim.enable_timers(False)
            first = sim.map(*look)
            for _ in range(2):
                assert sim.step() == 1
            out[rank] = (first, sim.map(*look), sim.sizes())
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
    ref, a, b = one[0][0], two[0][0], two[1][0]
    assert ref["grid"].shape == tuple((list(look[0]) + [1] * (3 - dim))[::-1]) + (11,)
    assert not np.isnan(ref["rows"]).any() and ref["rows"][:, 0].sum() == npts and ref["n_excluded"] == 0 and ref["outside"][0] == 0
    assert ref["rows"][:, 2].sum() > 0 and ref["rows"][:, 3].sum() > 0 and (ref["rows"][1:, 0] > 0).all()
    assert np.array_equal(a["rows"].view(np.uint64), ref["rows"].view(np.uint64))
    assert np.array_equal(b["rows"].view(np.uint64), ref["rows"].view(np.uint64))
    assert a["n_excluded"] == b["n_excluded"] == 0
    a, b = two[0][1], two[1][1]
    assert not np.isnan(a["rows"]).any() and np.array_equal(a["rows"].view(np.uint64), b["rows"].view(np.uint64))
    assert a["rows"][:, 0].sum() == npts and a["rows"][:, 4].sum() > 0 and np.abs(a["rows"][:, 5:5 + dim]).sum(axis=0).min() > 0


BREAKS3 = [[0, .3, .7, 1], [0, .5, 1], [0, .4, 1]]          # 12 zones (test_gpu_diagnostics)
EDGE_GRID = ("edge", (6, 4, 3), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


@pytest.fixture(scope="module")
def edge():
    from helpers import make_gpu
    from oracle.fem import Problem
    prob = Problem(breaks=BREAKS3, order_v=2, order_e=1, problem=1)
    gpu = make_gpu(prob)
    m = gpu.ctx.rho0DetJ0w

    def look(S, g):
        p = gpu.map(gpu.ctx.to_dev(S), g[1], g[2], g[3])
        ref = mr.map_reference(3, prob.NE, prob.N, prob.D1D, prob.L1D, np.asarray(prob.h1map).reshape(-1), S, m, prob.initial_state()[2],
                               prob.W, prob.B, prob.G, prob.Bl, g[1], g[2], g[3])
        return p, ref
    yield prob, look
    gpu.close()


def test_edge_inverted_layer(edge):
    import edge_states as es
    prob, look = edge
    p, ref = look(es.edge_state(prob, "inverted_layer"), EDGE_GRID)
    assert mr.undecided(ref) == 0
    assert ref["n_excluded"] > 0 and ref["n_excluded"] % prob.NQ == 0          # whole zones: the reflected layer
    check_rows(3, prob.ND, p["rows"], p["n_excluded"], ref, "inverted layer")
    assert p["rows"][:, 0].sum() == prob.NE * prob.NQ - ref["n_excluded"]
    assert np.all(p["rows"][:, 1] >= 0) and np.all(p["rows"][p["rows"][:, 0] > 0, 9] > 0)   # no negative volume, no negative density


def test_edge_all_negative_e(edge):
    import edge_states as es
    prob, look = edge
    p, ref = look(es.edge_state(prob, "all_negative_e"), EDGE_GRID)
    assert mr.undecided(ref) == 0
    check_rows(3, prob.ND, p["rows"], p["n_excluded"], ref, "all negative e")
    full = p["rows"][:, 0] > 0
    assert np.all(p["rows"][:, 8] == 0.0) and np.all(p["rows"][full, 3] < 0) and p["n_excluded"] == 0


def test_a_nan_coordinate_stays_in_its_zones(cases):
    """one y coordinate of one node of 3 x 2 x 2 zones is NaN: the points of the zones that hold the node are excluded, and
    nothing else - every column of every row stays finite and is the reference's"""
    c = cases("3D-3x2x2", (2, 1))
    hm = c.h1map.reshape(c.NE, c.ND)
    node = hm[5, 0]                                     # a corner of zone 5: shared
    holders = np.nonzero((hm == node).any(axis=1))[0]
    assert 1 < len(holders) < c.NE
    S = c.S.copy()
    S[c.N + node] = np.nan                              # its y coordinate
    Sd = c.ctx.to_dev(S)
    for name in ("unit", "partial", "one"):
        g = mc.grid(name, 3)
        p = run(c, g, Sd)
        ref = reference(c, g, S)
        assert p["n_excluded"] == len(holders) * c.NQ + reference(c, g)["n_excluded"]
        assert np.isfinite(p["rows"][:, :9]).all()
        check_rows(c.dim, c.ND, p["rows"], p["n_excluded"], ref, "NaN coordinate " + name)


def test_an_overflowing_addend_poisons_its_entry_only(cases):
    """the interior node of one Q2Q1 zone moves at 1e200: m |v|^2 overflows at every point of that zone (finite factors); the ke
    of the cells that hold such a point is NaN, their other columns are the reference's, and the next call on the clean state
    is clean"""
    c = cases("3D-3x2x2", (2, 1))
    g = mc.grid("unit", 3)
    clean = run(c, g, raw=True)
    hm = c.h1map.reshape(c.NE, c.ND)
    node = hm[5, 13]                                    # the middle node of 3 x 3 x 3
    assert (hm == node).sum() == 1
    S = c.S.copy()
    for k in range(3):
        S[(3 + k) * c.N + node] = 1e200
    ref = reference(c, g, S)
    bad = np.nonzero(np.isnan(ref["rows"][:, 4]))[0]
    assert 1 <= len(bad) < ref["rows"].shape[0] // 2 and np.isfinite(ref["rows"][:, [1, 2, 3, 5, 6, 7, 8]]).all()
    p = run(c, g, c.ctx.to_dev(S))
    assert np.isnan(p["rows"][bad, 4]).all() and np.isnan(p["rows"]).sum() == len(bad)
    check_rows(c.dim, c.ND, p["rows"], p["n_excluded"], ref, "overflow", rows=bad, skip={(r, 4) for r in bad})
    # the other cells keep their sums - but for the momentum columns, whose window sits under the largest addend of the whole
    # call, m 1e200: addends of order one are 2^-670 of that, below the 224 bits the two sets hold
    good = np.setdiff1d(np.arange(ref["rows"].shape[0]), bad)
    check_rows(c.dim, c.ND, p["rows"], p["n_excluded"], ref, "beside the overflow", rows=good, skip={(r, k) for r in good for k in (5, 6, 7)})
    assert np.array_equal(clean, run(c, g, raw=True))


def test_quiet_mesh_around_one_loud_zone(cases):
    """e and v scaled by 1e-12 everywhere but in one zone: ke addends of the quiet cells are 2^-80 of the largest; every row
    still meets the bounds relative to its own sum |addend|"""
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
    for name in ("unit", "fine"):
        g = mc.grid(name, 3)
        ref, p = reference(c, g, S), run(c, g, Sd)
        assert mr.undecided(ref) == 0
        ke = ref["abs"][1:, 4]
        assert ke[ke > 0].min() < 1e-20 * ke.max(), name        # quiet cells exist: whole cells lie away from the loud zone
        check_rows(c.dim, c.ND, p["rows"], p["n_excluded"], ref, "quiet mesh " + name)


def test_nothing_else_moves():
    """a map taken between two steps must not change the next step (test_gpu_diagnostics.test_nothing_else_moves)"""
    from helpers import deformed_state, make_gpu
    from oracle.fem import Problem
    prob = Problem(mesh="cube01_hex", rs=1, order_v=3, order_e=2, problem=1)
    gpu = make_gpu(prob)
    try:
        ctx = gpu.ctx
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
        p = ctx.map(Sd, (8, 8, 8), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
        q = gpu.map(Sd, (3, 50, 7), (-0.5, 0.0, 0.25), (1.5, 1.0, 0.75))
        assert p["rows"][:, 2].sum() > 0 and q["rows"][:, 0].sum() + q["n_excluded"] == prob.NE * prob.NQ
        assert ctx.quadrature_generation() == gen and ctx.get_dt_est() == dt
        assert np.array_equal(Sd.cpu().numpy(), S)
        after = products()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    finally:
        gpu.close()


def test_a_regrow_and_a_smaller_grid_after_it(cases):
    """a cell count that needs more scratch memory than the calls before it, then a smaller one: the rows of either are those of
    a context that has seen nothing else"""
    from test_gpu_diagnostics import Case
    c = cases("2D-3x2", (2, 1))
    small, large = ("small", (3, 2), (0.0, 0.0), (1.0, 1.0)), ("large", (300, 200), (0.0, 0.0), (1.0, 1.0))
    fresh = Case(mc.ZONES["2D-3x2"], 2, 1).setup()
    try:
        want_large, want_small = run(fresh, large, raw=True), run(fresh, small, raw=True)
    finally:
        fresh.close()
    assert np.array_equal(run(c, small, raw=True), want_small)
    assert np.array_equal(run(c, large, raw=True), want_large)
    assert np.array_equal(run(c, small, raw=True), want_small)
    p = run(c, large)
    assert p["rows"][:, 0].sum() + p["n_excluded"] == c.NE * c.NQ and p["rows"].shape == (60001, 11)


def test_refusals():
    """LGH_ERR_ARG (error 1) and no launch: before the set-up, and for every bad grid; the context is still usable afterwards"""
    import ctypes
    from laghos_amd import _lib
    from laghos_amd._lib import LghError
    from test_gpu_diagnostics import Case
    c = Case(mc.ZONES["2D-3x2"], 2, 1)
    try:
        Sd = c.ctx.to_dev(c.S)
        unit = ((7, 5), (0.0, 0.0), (1.0, 1.0))
        with pytest.raises(LghError, match="error 1: .*lgh_setup_rho0detj0"):
            c.ctx.map(Sd, *unit)
        c.setup()
        good = c.ctx.map(c.Sd, *unit)
        assert good["rows"][:, 0].sum() + good["n_excluded"] == c.NE * c.NQ
        inf, nan = float("inf"), float("nan")
        bad = [((0, 5), (0.0, 0.0), (1.0, 1.0)), ((7, -1), (0.0, 0.0), (1.0, 1.0)), ((7, 5, 2), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
               ((1024, 1025), (0.0, 0.0), (1.0, 1.0)), ((1 << 20, 2), (0.0, 0.0), (1.0, 1.0)), ((1 << 16, 1 << 16), (0.0, 0.0), (1.0, 1.0)),
               ((7, 5), (1.0, 0.0), (1.0, 1.0)), ((7, 5), (0.0, 2.0), (1.0, 1.0)), ((7, 5), (nan, 0.0), (1.0, 1.0)),
               ((7, 5), (0.0, 0.0), (1.0, inf)), ((7, 5), (0.0, -inf), (1.0, 0.0)), ((7, 5), (-1e308, 0.0), (1e308, 1.0))]
        for cells, lo, hi in bad:
            with pytest.raises(LghError, match="error 1: "):
                c.ctx.map(c.Sd, cells, lo, hi)
        # the largest grid there is, and bounds above the dimension are ignored
        assert c.ctx.map(c.Sd, (1024, 1024), (0.0, 0.0), (1.0, 1.0))["rows"][:, 0].sum() + good["n_excluded"] == c.NE * c.NQ
        assert np.array_equal(c.ctx.map(c.Sd, (7, 5, 1), (0.0, 0.0, nan), (1.0, 1.0, -inf))["rows"].view(np.uint64), good["rows"].view(np.uint64))
        L = _lib.load()
        spec = _lib.LghMapSpec()
        for k in range(3):
            spec.n[k], spec.lo[k], spec.hi[k] = (7, 5, 1)[k], 0.0, 1.0
        out, n = np.zeros(36 * 11), ctypes.c_long(0)
        dp = out.ctypes.data_as(_lib.c_dbl_p)
        S_ptr = ctypes.c_void_p(c.Sd.data_ptr())
        for call in (lambda: L.lgh_map(c.ctx.h, None, ctypes.byref(spec), dp, ctypes.byref(n)),
                     lambda: L.lgh_map(c.ctx.h, S_ptr, None, dp, ctypes.byref(n)),
                     lambda: L.lgh_map(c.ctx.h, S_ptr, ctypes.byref(spec), None, ctypes.byref(n)),
                     lambda: L.lgh_map(c.ctx.h, S_ptr, ctypes.byref(spec), dp, None),
                     lambda: L.lgh_map(None, S_ptr, ctypes.byref(spec), dp, ctypes.byref(n))):
            assert call() == 1
        assert not out.any()
        assert L.lgh_map(c.ctx.h, S_ptr, ctypes.byref(spec), dp, ctypes.byref(n)) == 0
        assert np.array_equal(out.view(np.uint64), good["rows"].reshape(-1).view(np.uint64)) and n.value == good["n_excluded"]
    finally:
        c.close()
