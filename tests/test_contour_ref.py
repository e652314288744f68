"""tests/contour_ref.py, the numpy restatement of lgh_contour (include/laghos_hip.h), held to facts that do not depend on it:
the residual of every vertex, the pairing of primitive edges inside a zone, closed-form areas and lengths on the undeformed
unit box, and a scalar of small integers with many lattice points exactly on the value."""
import itertools

import numpy as np
import pytest

from contour_ref import RULES, box_lattice, contour_reference, gather_reference, measure, simplex_points

EPS = np.finfo(np.float64).eps


def smooth_scalar(dim, NE, R1, seed):
    """one smooth random function per zone on its lattice (zones are independent in the definition)"""
    rng = np.random.default_rng(seed)
    r = np.arange(R1) / (R1 - 1)
    g = np.meshgrid(*([r] * dim), indexing="ij")[::-1]   # x fastest in the flattened index
    out = []
    for _ in range(NE):
        c, w = rng.uniform(-1, 1, dim + 1), rng.uniform(1, 5, dim)
        f = c[-1] + sum(c[a] * np.sin(w[a] * g[a] + a) for a in range(dim)) + 0.3 * np.prod([np.cos(3 * x) for x in g], axis=0)
        out.append(f.reshape(-1))
    return np.concatenate(out)


CASES = [(2, 1, 2), (2, 3, 3), (2, 2, 9), (3, 1, 2), (3, 2, 3), (3, 2, 6), (3, 1, 9)]


@pytest.mark.parametrize("dim,NE,R1", CASES)
def test_vertices_lie_on_the_value(dim, NE, R1):
    s = smooth_scalar(dim, NE, R1, 10 * dim + R1)
    for iso in (float(np.quantile(s, q)) for q in (0.3, 0.5, 0.72)):
        edges, t, zone, nskip = contour_reference(dim, NE, R1, s, iso)
        assert nskip == 0 and len(t) > 0
        s0, s1 = s[edges[..., 0]], s[edges[..., 1]]
        assert np.all(edges[..., 0] < edges[..., 1]) and np.all((s0 >= iso) != (s1 >= iso))
        assert np.all((t >= 0) & (t <= 1))
        res = np.abs(s0 + t * (s1 - s0) - iso)
        assert np.all(res <= 4 * EPS * np.maximum(np.maximum(np.abs(s0), np.abs(s1)), abs(iso)))
        # zones ascend, every edge lies in the zone its primitive names
        assert np.all(np.diff(zone) >= 0) and np.all(edges // R1 ** dim == zone[:, None, None])


def on_zone_boundary(dim, R1, pts):
    """the lattice points `pts` (..., n) of one zone lie in one boundary plane of the zone"""
    loc = pts % R1 ** dim
    hit = np.zeros(pts.shape[:-1], bool)
    for a in range(dim):
        r = (loc // R1 ** a) % R1
        hit |= np.all(r == 0, -1) | np.all(r == R1 - 1, -1)
    return hit


@pytest.mark.parametrize("dim,NE,R1", CASES)
def test_interior_edges_pair_with_opposite_sense(dim, NE, R1):
    s = smooth_scalar(dim, NE, R1, 77 + dim + R1)
    edges, t, zone, _ = contour_reference(dim, NE, R1, s, float(np.median(s)))
    n = len(edges)
    vid = edges[..., 0].astype(np.int64) * (NE * R1 ** dim) + edges[..., 1]          # a vertex is its lattice edge
    if dim == 2:
        # an end point inside the zone: once as the head of a segment, once as the tail of another
        inner = ~on_zone_boundary(2, R1, edges)
        tails, heads = vid[:, 0][inner[:, 0]], vid[:, 1][inner[:, 1]]
        assert len(tails) > 0 and len(np.unique(tails)) == len(tails) and len(np.unique(heads)) == len(heads)
        assert np.array_equal(np.sort(tails), np.sort(heads))
        return
    # directed primitive edges (A -> B) of every triangle; the lattice points of both vertices span a face of a tetrahedron
    A, B = vid, np.roll(vid, -1, axis=1)
    four = np.concatenate([edges, np.roll(edges, -1, axis=1)], axis=-1)                # (n, 3, 4)
    inner = ~on_zone_boundary(3, R1, four)
    fwd = np.stack([A[inner], B[inner]], 1)
    assert len(fwd) > 0
    keys, counts = np.unique(fwd, axis=0, return_counts=True)
    assert np.all(counts == 1), "a directed edge is used twice: two primitives with the same sense"
    rev = {(b, a) for a, b in keys.tolist()}
    assert rev == {(a, b) for a, b in keys.tolist()}, "an interior edge without its opposite"
    assert n > 0


def plane_scalar(X, normal):
    s = normal[0] * X[0]
    for a in range(1, len(normal)):
        s = s + normal[a] * X[a]
    return s


@pytest.mark.parametrize("zones", [(1, 1, 1), (2, 1, 3), (3, 2, 2), (3, 3, 3)])
@pytest.mark.parametrize("R1", [2, 3, 6, 9])
def test_hexagon_in_the_unit_cube(zones, R1):
    X = box_lattice(zones, R1)
    edges, t, zone, nskip = contour_reference(3, int(np.prod(zones)), R1, plane_scalar(X, (1.0, 1.0, 1.0)), 1.5)
    area = measure(gather_reference(edges, t, X))
    print(f"{zones} R1={R1}: {len(t)} triangles, area error {abs(area / (0.75 * np.sqrt(3.0)) - 1):.2e}")
    assert nskip == 0 and len(t) <= 11000      # (the bound's reasoning is for about 1e4 primitives)
    assert abs(area - 0.75 * np.sqrt(3.0)) <= 1e-12 * 0.75 * np.sqrt(3.0)


@pytest.mark.parametrize("zones", [(1, 1), (3, 2), (5, 7)])
@pytest.mark.parametrize("R1", [2, 3, 6, 9])
def test_segment_in_the_unit_square(zones, R1):
    X = box_lattice(zones, R1)
    edges, t, zone, nskip = contour_reference(2, int(np.prod(zones)), R1, plane_scalar(X, (1.0, 2.0)), 1.0)
    length = measure(gather_reference(edges, t, X))
    assert nskip == 0
    assert abs(length - 0.5 * np.sqrt(5.0)) <= 1e-12 * 0.5 * np.sqrt(5.0)
    # the inside (x + 2 y >= 1) to the left of every segment
    P = gather_reference(edges, t, X)
    d = P[:, :, 1] - P[:, :, 0]
    keep = np.hypot(*d) > 0
    assert np.all((d[0] * 2.0 - d[1] * 1.0)[keep] > 0)


def test_orientation_in_3d_points_out_of_the_inside():
    X = box_lattice((2, 2, 2), 4)
    nrm = np.array([0.3, -0.5, 0.8])
    edges, t, _, _ = contour_reference(3, 8, 4, plane_scalar(X, nrm), 0.2)
    P = gather_reference(edges, t, X)
    N = np.cross((P[:, :, 1] - P[:, :, 0]).T, (P[:, :, 2] - P[:, :, 0]).T)
    big = np.linalg.norm(N, axis=1) > 1e-12
    assert big.sum() > 50 and np.all((N @ nrm)[big] < 0)     # the scalar falls along the normal: inside -> outside is -grad s


def tie_scalar(dim, NE, R1, seed):
    return np.random.default_rng(seed).integers(0, 3, NE * R1 ** dim).astype(np.float64)


@pytest.mark.parametrize("dim,NE,R1", [(3, 1, 4), (3, 2, 5), (2, 1, 6), (2, 3, 5)])
def test_on_value_facets_come_exactly_once(dim, NE, R1):
    """Small integers, iso = 1: a third of the lattice points sit on the value.  A facet of a simplex whose corners all sit
    on the value is produced by the simplex on the side whose remaining corner is below - once per such simplex - and by no
    other; every vertex weight is 0, 1/2 or 1."""
    s = tie_scalar(dim, NE, R1, 5 + dim)
    iso = 1.0
    edges, t, zone, nskip = contour_reference(dim, NE, R1, s, iso)
    assert nskip == 0 and set(np.unique(t)) <= {0.0, 0.5, 1.0}
    # where the vertices sit, as lattice points (t = 1/2: none)
    at = np.where(t == 0.0, edges[..., 0], np.where(t == 1.0, edges[..., 1], -1))
    got = {}
    for prim in at:
        if prim.min() >= 0 and len(set(prim.tolist())) == dim:
            key = tuple(sorted(prim.tolist()))
            got[key] = got.get(key, 0) + 1
    want = {}
    for simplex in simplex_points(dim, NE, R1).reshape(-1, dim + 1):
        for drop in range(dim + 1):
            facet = np.delete(simplex, drop)
            if np.all(s[facet] == iso) and s[simplex[drop]] < iso:
                key = tuple(sorted(facet.tolist()))
                want[key] = want.get(key, 0) + 1
    assert len(want) > 3 and got == want


def test_a_value_that_is_not_finite_skips_its_simplices_only():
    dim, NE, R1 = 3, 2, 4
    s = smooth_scalar(dim, NE, R1, 3)
    iso = float(np.median(s))
    full = contour_reference(dim, NE, R1, s, iso)
    bad = s.copy()
    hole = 64 + 1 + 4 * (2 + 4 * 1)
    bad[hole] = np.nan
    edges, t, zone, nskip = contour_reference(dim, NE, R1, bad, iso)
    pts = simplex_points(dim, NE, R1).reshape(-1, dim + 1)
    touched = (pts == hole).any(1)
    assert nskip == touched.sum() > 0 and np.all(np.isfinite(t)) and not (edges == hole).any()
    # what is left is the full output in its order, bit for bit, less primitives that fit into a touched simplex
    sig = lambda e, tt: [(tuple(a.reshape(-1).tolist()), tuple(b.view(np.uint64).tolist())) for a, b in zip(e, tt)]
    left, everything = sig(edges, t), sig(full[0], full[1])
    it = iter(everything)
    assert all(any(x == y for y in it) for x in left), "not a subsequence of the full output"
    corner_sets = [set(p.tolist()) for p in pts[touched]]
    gone = set(everything) - set(left)
    assert len(gone) == len(everything) - len(left) > 0
    assert all(any(set(g[0]) <= cs for cs in corner_sets) for g in gone)


def test_the_rules_cover_every_case():
    for dim in (2, 3):
        perms, rules = RULES[dim]
        assert perms == sorted(itertools.permutations(range(dim)))
        for rk in rules:
            assert [len(r) for r in rk] == ([0, 1, 1, 1, 1, 1, 1, 0] if dim == 2 else [0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0])
