"""lgh_loads (Context.loads, HydroOperator.loads): pressure loads on lists of zone faces with exact, order-free sums, against
the numpy restatement of tests/loads_ref.py (held to the divergence theorem on the CPU by tests/test_loads_ref.py), the
outputs of lgh_sample_faces as a second witness, lgh_diagnostics, and edge states.

Shapes and orders are those of tests/test_gpu_faces.py; the states are helpers.deformed_state on helpers.CurvedInitialMesh
(loads_ref.case_data), with density dofs that vary.  Bound, everywhere (loads_ref.bound; none taken from what the kernel
gives): |got - want| <= 2 C kappa 2^-52 sum |addend| per (row, column); n and n_excluded exact; the extremes to
2 C 2^-52 pscale (loads_ref docstring).  "Same bits" compares the raw bytes of the rows.

The second witness: lgh_sample_faces takes the normal axis of a face at the first or last row of the lattice table it is
given, so the Gauss tables alone (R1 = Q1D) would put its points on the first Gauss plane inside the zone, not on the face.
The tables handed to it here are the Gauss rows with the two end-point rows around them (R1 = Q1D + 2), and the points with
an end-point row on a tangential axis are left out; where Q1D + 2 > 9 (Q4Q3) three calls with seven Gauss rows each cover
every pair of rows.

Launch edges: a face has NPF = Q1D^(dim-1) points, so lists of "63, 64 and 65 points" are the lists of 63 // NPF,
ceil(64 / NPF) and ceil(65 / NPF) faces - the nearest a whole number of faces comes to the end of a wavefront from either side.

An addend w p N_c that overflows takes w p |N| with it (|N| >= |N_c|): the overflow test holds the kernel to NaN in exactly
the entries where the reference has an addend that is not finite, two per row that lists the face.

Not covered: a face above 64 KB of LDS needs D1D = 10, for which no context can be created."""
import ctypes
import math

import numpy as np
import pytest

import loads_ref as lr

pytestmark = pytest.mark.gpu


class LoadsCase:
    def __init__(self, zones_id, order, W=None):
        from laghos_amd.context import Context
        self.zones_id, self.order = zones_id, order
        d = self.d = lr.case_data(lr.ZONES[zones_id], *order)
        self.dim, self.NE, self.N, self.D, self.L, self.Q = d["dim"], d["NE"], d["N"], d["D"], d["L"], d["Q"]
        self.NPF = self.Q ** (self.dim - 1)
        self.ctx = Context(self.dim, self.NE, self.D, self.Q, self.L, self.N, d["h1map"], d["B"], d["G"], d["Bl"], d["W"] if W is None else W,
                           d["gamma"], d["ess"], order_v=order[0])
        self.Sd, self.rhod = self.ctx.to_dev(d["S"]), self.ctx.to_dev(d["rho"])
        self.fp = lr.FacePoints(d)
        self.what = f"{zones_id} Q{order[0]}Q{order[1]}"

    def run(self, faces, nrows, Sd=None, rhod=None, raw=False):
        rows, n_excl = self.ctx.loads(self.Sd if Sd is None else Sd, self.rhod if rhod is None else rhod, faces, nrows)
        return (rows.view(np.uint64).copy(), n_excl) if raw else (rows, n_excl)

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(zones_id, order):
        key = (zones_id, order)
        if key not in made:
            made[key] = LoadsCase(zones_id, order)
        return made[key]
    yield get
    for c in made.values():
        c.close()


def check_rows(c, got, n_excl, ref, what, skip=()):
    """the bounds of the module docstring; prints the worst observed error over its bound"""
    want = ref["rows"]
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert n_excl == ref["n_excluded"], (what, n_excl, ref["n_excluded"])
    worst = 0.0
    for r in range(want.shape[0]):
        assert got[r, 0] == want[r, 0], (what, r, "n", got[r, 0], want[r, 0])
        for k in lr.SUM_COLS:
            if (r, k) in skip:
                continue
            if np.isnan(want[r, k]):
                assert np.isnan(got[r, k]), (what, r, lr.COLS[k], got[r, k])
                continue
            b = lr.bound(c.dim, c.D, c.L, ref["kappa"][r], ref["abs"][r, k])
            err = abs(got[r, k] - want[r, k])
            assert err <= b, (what, r, lr.COLS[k], got[r, k], want[r, k], err, b)
            if b > 0:
                worst = max(worst, err / b)
        for k in (9, 10):
            if np.isfinite(want[r, k]):
                assert abs(got[r, k] - want[r, k]) <= 2 * lr.C_ops(c.dim, c.D, c.L) * lr.EPS * ref["pscale"][r], (what, r, lr.COLS[k], got[r, k], want[r, k])
            else:
                assert got[r, k] == want[r, k], (what, r, lr.COLS[k], got[r, k], want[r, k])
        assert np.all(got[r, 2 + c.dim:5].view(np.uint64) == 0), (what, r, "a force component above the dimension")
    print(f"{what}: worst |got - want| / bound {worst:.4f}")


def plane_faces(c, axis, K):
    """the -pv-slice rule on the lexicographic mesh: side-0 faces of layer K, side-1 faces of the last layer for K = n"""
    n = c.d["zones"]
    idx = np.stack(np.unravel_index(np.arange(c.NE), n[::-1])[::-1], 1)     # (NE, dim): zone index per axis, x fastest
    layer, side = (K, 0) if K < n[axis] else (n[axis] - 1, 1)
    z = np.nonzero(idx[:, axis] == layer)[0]
    return np.stack([z, np.full(len(z), 2 * axis + side)], 1).astype(np.int32)


def groups_of(c):
    """the driver's rows and one more: surface, walls, a plane inside, every face of every zone"""
    g = lr.wall_groups(c.d, c.ctx.boundary_faces())
    a = c.dim - 1
    g.append((f"plane_{'xyz'[a]}", plane_faces(c, a, c.d["zones"][a] // 2 + (1 if c.d["zones"][a] > 1 else 0))))
    g.append(("all", lr.all_faces(c.d)))
    return g


@pytest.mark.parametrize("zones_id,order", lr.CASES, ids=lr.IDS)
def test_rows_match_numpy(cases, zones_id, order):
    c = cases(zones_id, order)
    assert np.array_equal(c.ctx.boundary_faces(), lr.boundary_faces(c.d))
    groups = groups_of(c)
    faces = lr.listing(groups)
    ref = lr.loads_reference(c.fp, faces, len(groups))
    rows, n_excl = c.run(faces, len(groups))
    check_rows(c, rows, n_excl, ref, c.what)
    assert n_excl == 0 and rows[:, 0].sum() == len(faces) * c.NPF and (rows[:, 1] > 0).all() and (rows[:, 9] <= rows[:, 10]).all()
    # the walls add up to the surface row
    nw = 2 * c.dim
    assert rows[1:1 + nw, 0].sum() == rows[0, 0]
    for k in lr.SUM_COLS:
        b = lr.bound(c.dim, c.D, c.L, ref["kappa"][:1 + nw].max(), 2 * ref["abs"][0, k])
        assert abs(rows[1:1 + nw, k].sum() - rows[0, k]) <= b, (c.what, lr.COLS[k])
    assert rows[0, 9] == rows[1:1 + nw, 9].min() and rows[0, 10] == rows[1:1 + nw, 10].max()


def witness_rows(c, faces, nrows):
    """the rows as math.fsum over x, v, p and area_normal of lgh_sample_faces at the Gauss points of the faces (module docstring)"""
    from derived_ref import lattice_tables3
    d, dim, Q = c.d, c.dim, c.Q
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    nf = len(faces)
    Eb, Eg, El = lattice_tables3(d["ok"], d["ot"], 1)
    subsets = [list(range(Q))] if Q + 2 <= 9 else [[q for q in range(Q) if q != k] for k in (0, Q - 1, 1)]
    runs = []
    for sub in subsets:
        tab = lambda E, T: np.vstack([E[0:1], T[sub], E[1:2]])
        R1 = len(sub) + 2
        NPL = R1 ** (dim - 1)
        out = {k: c.ctx.to_dev(np.full(n * nf * NPL, np.nan)) for k, n in (("x", dim), ("v", dim), ("p", 1), ("area_normal", dim))}
        c.ctx.sample_faces(c.Sd, c.rhod, tab(Eb, d["B"]), tab(Eg, d["G"]), tab(El, d["Bl"]), faces[:, :2], **out)
        c.ctx.sync()
        runs.append((sub, R1, {k: t.cpu().numpy().reshape(-1, nf, NPL) for k, t in out.items()}))
    add = [[[] for _ in range(8)] for _ in range(nrows)]
    w1 = d["w1"]
    for p in range(c.NPF):
        qs = (p,) if dim == 2 else (p % Q, p // Q)
        sub, R1, o = next(r for r in runs if all(q in r[0] for q in qs))
        lat = sum((1 + sub.index(q)) * R1 ** i for i, q in enumerate(qs))
        w = math.prod(w1[q] for q in qs)
        x, v, Nv, pr = o["x"][:, :, lat], o["v"][:, :, lat], o["area_normal"][:, :, lat], o["p"][0, :, lat]
        assert np.isfinite(x).all() and np.isfinite(v).all() and np.isfinite(Nv).all() and np.isfinite(pr).all()
        nrm = np.sqrt((Nv * Nv).sum(0))
        vn, xn, wp = (v * Nv).sum(0), (x * Nv).sum(0), w * pr
        cols = [w * nrm] + [wp * Nv[k] if k < dim else np.zeros(nf) for k in range(3)] + [wp * nrm, wp * vn, w * vn, w * xn]
        for i, r in enumerate(faces[:, 2]):
            for k in range(8):
                add[r][k].append(float(cols[k][i]))
    return np.array([[math.fsum(add[r][k]) for k in range(8)] for r in range(nrows)])


@pytest.mark.parametrize("zones_id,order", lr.CASES, ids=lr.IDS)
def test_rows_match_the_faces_kernel(cases, zones_id, order):
    c = cases(zones_id, order)
    groups = groups_of(c)
    faces = lr.listing(groups)
    ref = lr.loads_reference(c.fp, faces, len(groups))
    rows, _ = c.run(faces, len(groups))
    wit = witness_rows(c, faces, len(groups))
    worst = 0.0
    for r in range(len(groups)):
        for k in lr.SUM_COLS:
            b = lr.bound(c.dim, c.D, c.L, ref["kappa"][r], ref["abs"][r, k])
            err = abs(rows[r, k] - wit[r, k - 1])
            assert err <= b, (c.what, groups[r][0], lr.COLS[k], rows[r, k], wit[r, k - 1], err, b)
            worst = max(worst, err / b if b > 0 else 0.0)
    print(f"{c.what}: worst |loads - faces kernel| / bound {worst:.4f}")


@pytest.mark.parametrize("zones_id,order", lr.CASES, ids=lr.IDS)
def test_xn_of_the_surface_is_dim_times_the_volume(cases, zones_id, order):
    """against slot 1 of lgh_diagnostics, within the bound plus the diagnostics' own sum bound (tests/test_gpu_diagnostics.py:
    (terms + dim D1D^dim + 8) 2^-52 of the sum of |terms|, over the points of a zone and over the zones)"""
    c = cases(zones_id, order)
    d = c.d
    c.ctx.setup_rho0detj0(c.ctx.to_dev(d["x0"]), c.ctx.to_dev(d["rho0_l2"]), c.ctx.to_dev(d["rho0_q"]))
    vol = c.ctx.diagnostics(c.Sd, raw=True)[1]
    bf = c.ctx.boundary_faces()
    faces = np.concatenate([bf, np.zeros((len(bf), 1), np.int32)], 1)
    ref = lr.loads_reference(c.fp, faces, 1)
    rows, _ = c.run(faces, 1)
    _, vol_abs, _, _ = lr.volume_integrals(d)
    NQ, ND = c.Q ** c.dim, c.D ** c.dim
    b = lr.bound(c.dim, c.D, c.L, ref["kappa"][0], ref["abs"][0, 8]) + c.dim * ((NQ + c.dim * ND + 8) + (c.NE + c.dim * ND + 8)) * lr.EPS * vol_abs
    print(f"{c.what}: |xn - dim vol| / bound {abs(rows[0, 8] - c.dim * vol) / b:.4f}")
    assert vol > 0 and abs(rows[0, 8] - c.dim * vol) <= b, (rows[0, 8], c.dim * vol, b)


BITS = [("2D-3x2", (4, 3)), ("3D-5x5x3", (3, 2)), ("3D-3x2x2", (2, 1)), ("2D-3x2", (1, 0))]


@pytest.mark.parametrize("zones_id,order", BITS)
def test_same_bits_for_every_order_and_repetition(cases, zones_id, order):
    c = cases(zones_id, order)
    groups = groups_of(c)
    faces, n = lr.listing(groups), len(groups)
    first = c.run(faces, n, raw=True)
    assert np.array_equal(first[0], c.run(faces, n, raw=True)[0])
    rng = np.random.default_rng(11)
    for other in (faces[::-1], faces[rng.permutation(len(faces))]):
        got = c.run(np.ascontiguousarray(other), n, raw=True)
        assert np.array_equal(first[0], got[0]) and got[1] == first[1]
    # every face twice, under rows r and n + r: both halves are the rows of the list given once
    twice = np.concatenate([faces, faces + np.array([0, 0, n], np.int32)])
    got = c.run(twice[rng.permutation(len(twice))], 2 * n, raw=True)[0]
    assert np.array_equal(got[:n], first[0]) and np.array_equal(got[n:], first[0])
    # ... and twice under the SAME row: the count doubles; the exact sums do too, and come out through the dozen rounded additions
    # that join the limbs of a sum into a double (prof_value_k), so to 16 x 2^-52 of themselves
    rows2, _ = c.run(np.concatenate([faces, faces]), n)
    rows1 = first[0].view(np.float64)
    assert np.array_equal(rows2[:, 0], 2 * rows1[:, 0]) and np.array_equal(rows2[:, 9:], rows1[:, 9:])
    assert np.all(np.abs(rows2[:, 1:9] - 2 * rows1[:, 1:9]) <= 16 * lr.EPS * np.abs(2 * rows1[:, 1:9]))


@pytest.mark.parametrize("zones_id", ["3D-3x2x2", "2D-3x2"])
def test_same_bits_on_a_renumbered_mesh(cases, zones_id):
    """another numbering of nodes and zones (Discretization::Renumber) with the same tables and the same data: faces name the
    caller's zone ids, and the rows have the bytes of the lexicographic mesh"""
    from laghos_amd import host_lib
    from laghos_amd.context import Context
    c = cases(zones_id, (3, 2))
    d, dim, NE, N = c.d, c.dim, c.NE, c.N
    h = host_lib.host_disc("cartesian", 0, 3, 2, 1, zones=lr.ZONES[zones_id], renumber="random", seed=5)
    ep, npm = h["elem_perm"], h["node_perm"]        # renumbered zone j is lexicographic zone ep[j]; lexicographic node i is node npm[i]
    assert not np.array_equal(ep, np.arange(NE)) and not np.array_equal(npm, np.arange(N))
    inv, inv_node = np.argsort(ep), np.argsort(npm)
    assert np.array_equal(inv_node[h["h1map"].reshape(NE, -1)[inv]].reshape(-1), d["h1map"])     # the same mesh
    nodes = lambda a, ncomp: np.concatenate([a[k * N:(k + 1) * N][inv_node] for k in range(ncomp)])
    zones = lambda a, per: a.reshape(NE, per)[ep].reshape(-1)
    H1V, NL = dim * N, c.L ** dim
    S = np.concatenate([nodes(d["S"][:2 * H1V], 2 * dim), zones(d["S"][2 * H1V:], NL)])
    ren = Context(dim, NE, c.D, c.Q, c.L, N, h["h1map"], d["B"], d["G"], d["Bl"], d["W"], d["gamma"][ep], h["ess"], order_v=3)
    try:
        groups = groups_of(c)
        faces = lr.listing(groups)
        want = c.run(faces, len(groups), raw=True)
        there = faces.copy()
        there[:, 0] = inv[faces[:, 0]]
        rows, n_excl = ren.loads(ren.to_dev(S), ren.to_dev(zones(d["rho"], NL)), there, len(groups))
        assert np.array_equal(rows.view(np.uint64), want[0]) and n_excl == want[1]
        # the boundary found from the renumbered map is the same set of faces
        bf = ren.boundary_faces()
        assert sorted(map(tuple, np.stack([ep[bf[:, 0]], bf[:, 1]], 1).tolist())) == sorted(map(tuple, lr.boundary_faces(d).tolist()))
    finally:
        ren.close()


@pytest.mark.parametrize("pgrid,order", [((2, 1), (2, 1)), ((2, 1, 1), (2, 1))], ids=["2D", "3D"])
def test_two_emulated_ranks_against_one(pgrid, order):
    """the global problem on one rank against its two halves on two (tests/rank_threads.py): every rank lists the faces of its
    own zones - the walls of the global box and a plane that lies on the second rank only - and both return the bytes of
    the one-rank call"""
    import rank_cases as rc
    from helpers import deformed_state, make_gpu
    from rank_threads import Ranks
    glob, probs = rc.problems(pgrid, "equal", order)
    dim = glob.dim
    Sg = deformed_state(glob, seed=9)
    rho_g = np.random.default_rng(4).uniform(0.5, 2.0, glob.L2V)
    from laghos_amd.context import boundary_faces_host
    bf = boundary_faces_host(dim, glob.NE, glob.N, glob.D1D, np.asarray(glob.h1map).reshape(-1))
    ne = rc.global_shape(pgrid)
    idx = np.stack(np.unravel_index(np.arange(glob.NE), ne[::-1])[::-1], 1)
    K = ne[0] - 2                                                     # an x-plane inside the second rank
    pl = np.nonzero(idx[:, 0] == K)[0]
    groups = [("surface", bf)] + [("w", bf[bf[:, 1] == f]) for f in range(2 * dim)] + [("plane", np.stack([pl, np.zeros(len(pl), int)], 1))]
    faces, n = lr.listing(groups), len(groups)
    one = make_gpu(glob)
    try:
        want, want_excl = one.ctx.loads(one.ctx.to_dev(Sg), one.ctx.to_dev(rho_g), faces, n)
    finally:
        one.close()
    assert want_excl == 0 and (want[:, 0] > 0).all() and not np.isnan(want).any()
    ranks = Ranks(probs)
    try:
        def leg(r, op, p):
            local = -np.ones(glob.NE, np.int64)
            zm = rc.zone_map(p)
            local[zm] = np.arange(p.NE)
            mine = faces[local[faces[:, 0]] >= 0].copy()
            mine[:, 0] = local[mine[:, 0]]
            rows, n_excl = op.ctx.loads(op.ctx.to_dev(rc.slice_state(p, Sg)), op.ctx.to_dev(rc.slice_zones(p, rho_g, p.NL)), mine, n)
            return rows, n_excl, len(mine), int((mine[:, 2] == n - 1).sum())
        got = ranks.run(leg)
    finally:
        ranks.close()
    assert got[0][2] + got[1][2] == len(faces) and got[0][3] == 0 and got[1][3] == len(pl)
    for rows, n_excl, _, _ in got:
        assert np.array_equal(rows.view(np.uint64), want.view(np.uint64)) and n_excl == 0


@pytest.mark.parametrize("zones_id,order", [("3D-5x5x3", (1, 0)), ("3D-5x5x3", (3, 2)), ("2D-3x2", (1, 0)), ("2D-3x2", (4, 3)), ("3D-3x2x2", (2, 1)),
                                            ("3D-1x1x1", (4, 3))])
def test_launch_edges(cases, zones_id, order):
    c = cases(zones_id, order)
    every = lr.all_faces(c.d)
    cyc = lambda n: every[(np.arange(n) * 5 + 1) % len(every)]      # n faces, zones not consecutive, repeats once n > len
    fpb = c.ctx.loads_faces_per_block()
    assert 1 <= fpb <= 256 // c.NPF
    lists = {"one": every[[len(every) // 2]], "zone": every[every[:, 0] == c.NE // 2]}
    for n in sorted({63 // c.NPF, -(-64 // c.NPF), -(-65 // c.NPF), fpb - 1, fpb, fpb + 1}):
        if n > 0:
            lists[f"{n} faces ({n * c.NPF} points)"] = cyc(n)
    for name, fl in lists.items():
        nrows = 3
        faces = np.concatenate([fl, (np.arange(len(fl))[:, None] % nrows)], 1).astype(np.int32)
        rows, n_excl = c.run(faces, nrows)
        check_rows(c, rows, n_excl, lr.loads_reference(c.fp, faces, nrows), f"{c.what} FPB {fpb} {name}")
    # no face at all: empty rows
    rows, n_excl = c.run(np.zeros((0, 3), np.int32), 5)
    assert n_excl == 0 and np.all(rows[:, :9].view(np.uint64) == 0) and np.all(np.isposinf(rows[:, 9])) and np.all(np.isneginf(rows[:, 10]))
    # the most rows there are, more than a wavefront folds: every face under its own row where they last
    faces = np.concatenate([every, (np.arange(len(every))[:, None] * 7 % 64)], 1).astype(np.int32)
    rows, n_excl = c.run(faces, 64)
    check_rows(c, rows, n_excl, lr.loads_reference(c.fp, faces, 64), f"{c.what} 64 rows")


def test_a_nan_coordinate_excludes_the_faces_that_hold_the_node(cases):
    """one y coordinate of a corner node of zone 5 of 3 x 2 x 2 zones is NaN: the points of the faces that hold the node - three of
    zone 5, and those of its neighbours that share it - are excluded, as the reference counts them, and nothing else moves"""
    from faces_ref import face_nodes
    c = cases("3D-3x2x2", (2, 1))
    hm = c.d["h1map"].reshape(c.NE, -1)
    node = hm[5, 0]
    faces = np.concatenate([lr.all_faces(c.d), np.zeros((6 * c.NE, 1), np.int32)], 1)
    faces[:, 2] = faces[:, 1] % 2
    holders = [(e, f) for e, f, _ in faces if node in hm[e, face_nodes(3, c.D, f)]]
    assert len(holders) > 3 and len({e for e, _ in holders}) > 1
    S = c.d["S"].copy()
    S[c.N + node] = np.nan
    ref = lr.loads_reference(lr.FacePoints(c.d, S=S), faces, 2)
    assert ref["n_excluded"] == len(holders) * c.NPF
    rows, n_excl = c.run(faces, 2, Sd=c.ctx.to_dev(S))
    assert np.isfinite(rows).all()
    check_rows(c, rows, n_excl, ref, "NaN coordinate")
    # a NaN energy: the faces of that zone only
    S = c.d["S"].copy()
    S[2 * 3 * c.N + 5 * c.L ** 3] = np.nan
    ref = lr.loads_reference(lr.FacePoints(c.d, S=S), faces, 2)
    assert ref["n_excluded"] == 3 * c.NPF
    rows, n_excl = c.run(faces, 2, Sd=c.ctx.to_dev(S))
    check_rows(c, rows, n_excl, ref, "NaN energy")


def test_all_negative_e(cases):
    import edge_states as es
    c = cases("3D-3x2x2", (2, 1))
    prob = c.d["prob"]
    groups = lr.wall_groups(c.d)
    faces = lr.listing(groups)
    S = es.edge_state(prob, "all_negative_e")
    Spos = S.copy()
    Spos[2 * prob.H1V:] = 1.0
    rows, n_excl = c.run(faces, len(groups), Sd=c.ctx.to_dev(S))
    base, _ = c.run(faces, len(groups), Sd=c.ctx.to_dev(Spos))
    assert n_excl == 0 and np.all(rows[:, 2:7] == 0.0) and np.all(rows[:, 10] == 0.0) and np.all(rows[:, 9] == 0.0)
    assert np.array_equal(rows[:, [0, 1, 7, 8]].view(np.uint64), base[:, [0, 1, 7, 8]].view(np.uint64)) and (base[:, 5] > 0).all()
    check_rows(c, rows, n_excl, lr.loads_reference(lr.FacePoints(c.d, S=S), faces, len(groups)), "all negative e")


def test_an_overflowing_addend_poisons_its_entries_only(cases):
    """the unit box scaled by 1000 with flat faces (N has one component, the others are exact zeros), v = 0 on the nodes of zone
    0 and e = 1e308 in it: on its face x0 every w p N_x and w p |N| overflows from finite factors.  That face stands alone in
    row 1 and with the wall in row 0: NaN in exactly the entries where the reference has an addend that is not finite, every
    other entry within the bound; the next call on the clean state is clean"""
    c = cases("3D-3x2x2", (2, 1))
    d, prob = c.d, c.d["prob"]
    H1V, NL = prob.H1V, c.L ** 3
    S = d["S"].copy()
    S[:H1V] = 1000.0 * prob.initial_state()[0][:H1V]
    hm = d["h1map"].reshape(c.NE, -1)
    for k in range(3):
        S[H1V + k * c.N + hm[0]] = 0.0
    S[2 * H1V:2 * H1V + NL] = 1e308
    bf = lr.boundary_faces(d)
    x0 = bf[bf[:, 1] == 0]
    rest = bf[bf[:, 1] != 0]
    groups = [("x0", x0), ("hot", np.array([[0, 0]], np.int32)), ("rest", rest[rest[:, 0] != 0])]
    faces = lr.listing(groups)
    ref = lr.loads_reference(lr.FacePoints(d, S=S), faces, 3)
    nan = np.argwhere(np.isnan(ref["rows"]))
    assert sorted(map(tuple, nan.tolist())) == [(0, 2), (0, 5), (1, 2), (1, 5)] and np.isfinite(ref["rows"][:, 10]).all()
    clean = c.run(faces, 3, raw=True)
    rows, n_excl = c.run(faces, 3, Sd=c.ctx.to_dev(S))
    assert np.array_equal(np.argwhere(np.isnan(rows)), nan)
    check_rows(c, rows, n_excl, ref, "overflow")
    assert np.array_equal(c.run(faces, 3, raw=True)[0], clean[0])


def test_a_negative_density_gives_a_negative_p_min(cases):
    for zones_id, order in (("3D-3x2x2", (2, 1)), ("2D-3x2", (3, 2))):
        c = cases(zones_id, order)
        groups = lr.wall_groups(c.d)
        faces = lr.listing(groups)
        rho = c.d["rho"].copy()
        rho[0] = -3.0                              # the first dof of zone 0: its corner on the walls x0, y0 (z0)
        ref = lr.loads_reference(lr.FacePoints(c.d, rho=rho), faces, len(groups))
        assert ref["rows"][0, 9] < 0 < ref["rows"][0, 10] and (ref["rows"][[2, 4], 9] > 0).all() and ref["rows"][1, 9] < 0
        rows, n_excl = c.run(faces, len(groups), rhod=c.ctx.to_dev(rho))
        check_rows(c, rows, n_excl, ref, f"{c.what} negative density")
        assert rows[0, 9] < 0 and rows[0, 9] == rows[1:, 9].min()
        # all pressures negative or zero in a row: the maximum is negative too
        neg = -c.d["rho"]
        ref = lr.loads_reference(lr.FacePoints(c.d, rho=neg), faces, len(groups))
        rows, n_excl = c.run(faces, len(groups), rhod=c.ctx.to_dev(neg))
        check_rows(c, rows, n_excl, ref, f"{c.what} all densities negative")
        assert (rows[:, 10] <= 0).all() and (rows[:, 9] < 0).all()


def test_nothing_else_moves():
    """loads taken between two steps must not change the next step (test_gpu_map.test_nothing_else_moves); and what
    HydroOperator.loads returns"""
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
        gen, dt, fp = ctx.quadrature_generation(), ctx.get_dt_est(), ctx.fingerprint(Sd)
        assert gen[1] == 1 and gen[2] == 1 and np.isfinite(dt)
        bf = ctx.boundary_faces()
        groups = [("surface", bf), ("x0", bf[bf[:, 1] == 0]), ("empty", np.zeros((0, 2), np.int32))]
        out = gpu.loads(Sd, groups)
        rho = gpu.compute_density(Sd)
        rows, n_excl = ctx.loads(Sd, rho, lr.listing(groups[:2]), 3)
        assert out["names"] == ["surface", "x0", "empty"] and np.array_equal(out["rows"].view(np.uint64), rows.view(np.uint64)) and out["n_excluded"] == n_excl == 0
        assert out["force"].shape == (3, 3) and np.array_equal(out["force"], rows[:, 2:5])
        assert np.array_equal(out["p_mean"][:2], rows[:2, 5] / rows[:2, 1]) and np.isnan(out["p_mean"][2])
        assert rows[0, 0] == len(bf) * 36 and rows[2, 0] == 0 and np.isposinf(rows[2, 9]) and np.isneginf(rows[2, 10])
        assert ctx.quadrature_generation() == gen and ctx.get_dt_est() == dt and ctx.fingerprint(Sd) == fp
        assert np.array_equal(Sd.cpu().numpy(), S)
        after = products()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    finally:
        gpu.close()


def test_refusals(cases):
    """every refusal returns its code, names the value, launches nothing, and a valid call after it gives the bits of before"""
    from laghos_amd import _lib
    from laghos_amd._lib import LghError
    c = cases("3D-3x2x2", (2, 1))
    L = _lib.load()
    groups = lr.wall_groups(c.d)
    faces, n = lr.listing(groups), len(groups)
    good = c.run(faces, n, raw=True)

    def refused(code, match, fc=faces, nrows=n):
        with pytest.raises(LghError, match=f"error {code}: .*{match}") as ei:
            c.ctx.loads(c.Sd, c.rhod, fc, nrows)
        assert str(ei.value).split(": ", 1)[1] == L.lgh_last_error().decode()
        assert np.array_equal(c.run(faces, n, raw=True)[0], good[0])

    refused(1, "nrows = 0 ", nrows=0)
    refused(1, "nrows = 65 ", nrows=65)
    refused(1, "nrows = -3 ", nrows=-3)
    for col, bad, match in ((0, c.NE, f"zone {c.NE} "), (0, -1, "zone -1 "), (1, 6, "local face 6 "), (1, -2, "local face -2 "), (2, n, f"row {n} "),
                            (2, -1, "row -1 ")):
        fc = faces.copy()
        fc[7, col] = bad
        refused(1, match, fc=fc)
    # NULL arguments and nfaces < 0: through the library itself
    out, ne = np.full(n * 11, np.nan), ctypes.c_long(-7)
    S, rho = ctypes.c_void_p(c.Sd.data_ptr()), ctypes.c_void_p(c.rhod.data_ptr())
    fp, dp, nep = faces.ctypes.data_as(_lib.c_int_p), out.ctypes.data_as(_lib.c_dbl_p), ctypes.byref(ne)
    for args, match in (((c.ctx.h, None, rho, n, len(faces), fp, dp, nep), b"S is NULL"), ((c.ctx.h, S, None, n, len(faces), fp, dp, nep), b"rho_l2 is NULL"),
                        ((c.ctx.h, S, rho, n, len(faces), None, dp, nep), b"faces is NULL"), ((c.ctx.h, S, rho, n, len(faces), fp, None, nep), b"out is NULL"),
                        ((c.ctx.h, S, rho, n, len(faces), fp, dp, None), b"n_excluded is NULL"), ((c.ctx.h, S, rho, n, -1, fp, dp, nep), b"nfaces = -1"),
                        ((None, S, rho, n, len(faces), fp, dp, nep), b"bad argument")):
        assert L.lgh_loads(*args) == 1 and match in L.lgh_last_error(), match
        assert np.isnan(out).all() and ne.value == -7
    assert L.lgh_loads(c.ctx.h, S, rho, n, len(faces), fp, dp, nep) == 0 and ne.value == 0
    assert np.array_equal(out.view(np.uint64), good[0].reshape(-1))
    fpb = ctypes.c_int(-1)
    assert L.lgh_loads_fpb(c.ctx.h, None) == 1 and L.lgh_loads_fpb(None, ctypes.byref(fpb)) == 1 and fpb.value == -1
    # 1D: refused
    from test_gpu_sample import Case
    c1 = Case((3,), 2, 1)
    try:
        with pytest.raises(LghError, match="error 1: .*dim = 1"):
            c1.ctx.loads(c1.Sd, c1.rhod, np.array([[0, 0, 0]], np.int32), 1)
        with pytest.raises(LghError, match="error 1: .*dim = 1"):
            c1.ctx.loads_faces_per_block()
    finally:
        c1.close()
    # a rule that is no tensor product of a 1-D rule: unsupported, the context stays usable otherwise
    W = c.d["W"].copy()
    W[1] *= 1.5
    odd = LoadsCase("3D-3x2x2", (2, 1), W=W)
    try:
        with pytest.raises(LghError, match="error 2: .*Q1D = 4.*not a tensor product"):
            odd.run(faces, n)
        with pytest.raises(LghError, match="error 2: "):
            odd.ctx.loads_faces_per_block()
        assert len(odd.ctx.boundary_faces()) == len(groups[0][1])
    finally:
        odd.close()
