"""The contour stage (lgh_contour, include/laghos_hip.h) restated in numpy: marching tetrahedra (3D) / marching triangles (2D)
over the lattice of lgh_sample_fields, from the rules of the definition - no case table is written down here: the primitives of
a simplex and their sense are worked out from the corner positions for every (simplex, inside set) when the module loads.

    lattice      NP = NE * R1^dim values, pt = e * R1^dim + rx + R1 * (ry + R1 * rz); inside: scalar[pt] >= iso
    sub-cell     lower corner (rx, ry, rz), r* < R1 - 1, index rx + (R1-1) * (ry + (R1-1) * rz)
    simplex k    the path 000 -> e_a -> e_a + e_b -> 111 of the k-th permutation (a, b[, c]) of the axes, lexicographic;
                 corners 0..dim in path order (their lattice indices ascend along the path)
    vertex       on a lattice edge (p0 < p1) whose ends differ in side, t = (iso - s[p0]) / (s[p1] - s[p0])
    primitives   one inside corner a, outside o1 < o2 [< o3]:   (a o1, a o2[, a o3])
                 one outside corner o, inside i1 < i2 [< i3]:   (i1 o, i2 o[, i3 o])
                 3D, inside a < b, outside c < d:               (ac, ad, bd), (ac, bd, bc)
                 the last two vertices swapped where the sense is the other one: 3D the normal (right-hand rule, lattice
                 coordinates) points from the inside corners to the outside ones; 2D the inside lies to the left
    skipped      a simplex with a non-finite corner value: nothing, counted
    order        (zone, sub-cell, simplex, primitive) ascending"""
import itertools

import numpy as np


def simplex_corners(perm):
    """corner positions (dim + 1, dim) of the path of the permutation, as integers"""
    dim = len(perm)
    c = np.zeros((dim + 1, dim), np.int64)
    for i, a in enumerate(perm):
        c[i + 1] = c[i]
        c[i + 1, a] += 1
    return c


def simplex_rule(perm, inside):
    """The primitives of one simplex: a list of primitives, each a list of dim vertices (i, j), i < j corners in path order.
    `inside`: dim + 1 booleans."""
    dim = len(perm)
    I = [i for i in range(dim + 1) if inside[i]]
    O = [i for i in range(dim + 1) if not inside[i]]
    if not I or not O:
        return []
    if len(I) == 1:
        prims = [[(I[0], o) for o in O]]
    elif len(O) == 1:
        prims = [[(i, O[0]) for i in I]]
    else:
        (a, b), (c, d) = I, O
        prims = [[(a, c), (a, d), (b, d)], [(a, c), (b, d), (b, c)]]
    X = simplex_corners(perm).astype(float)
    mid = lambda v: 0.5 * (X[v[0]] + X[v[1]])
    out_dir = X[O].mean(0) - X[I].mean(0)
    res = []
    for p in prims:
        P = [mid(v) for v in p]
        if dim == 3:
            sense = np.dot(np.cross(P[1] - P[0], P[2] - P[0]), out_dir)
        else:   # the inside to the left of P0 -> P1: the outside to the right
            d = P[1] - P[0]
            sense = d[1] * out_dir[0] - d[0] * out_dir[1]
        assert abs(sense) > 1e-6
        if sense < 0:
            p = p[:-2] + [p[-1], p[-2]]
        res.append([(min(v), max(v)) for v in p])
    return res


def _rules(dim):
    perms = list(itertools.permutations(range(dim)))   # lexicographic
    return perms, [[simplex_rule(perm, [(m >> i) & 1 for i in range(dim + 1)]) for m in range(1 << (dim + 1))] for perm in perms]


RULES = {2: _rules(2), 3: _rules(3)}


def simplex_points(dim, NE, R1):
    """Lattice indices of the corners of every simplex: (NE, NSC, nsimp, dim + 1), in the order of the definition"""
    C = R1 - 1
    NPZ = R1 ** dim
    r = np.arange(C)
    if dim == 3:
        rz, ry, rx = np.meshgrid(r, r, r, indexing="ij")
    else:
        ry, rx = np.meshgrid(r, r, indexing="ij")
        rz = np.zeros_like(rx)
    base = (rx + R1 * (ry + R1 * rz)).reshape(-1)                     # ascending sub-cell index
    stride = np.array([1, R1, R1 * R1][:dim])
    perms, _ = RULES[dim]
    off = np.array([simplex_corners(p) @ stride for p in perms])      # (nsimp, dim + 1)
    loc = base[:, None, None] + off[None, :, :]
    return (np.arange(NE)[:, None, None, None] * NPZ + loc[None]).astype(np.int64)


def contour_reference(dim, NE, R1, scalar, iso):
    """(edges (n, dim, 2) int32, t (n, dim) float64, zone (n,) int32, n_skipped)"""
    scalar = np.asarray(scalar, np.float64).reshape(-1)
    assert dim in (2, 3) and 2 <= R1 <= 9 and scalar.size == NE * R1 ** dim
    iso = np.float64(iso)
    pts = simplex_points(dim, NE, R1)
    shape = pts.shape[:3]
    nsimp = shape[2]
    pts = pts.reshape(-1, dim + 1)
    val = scalar[pts]
    finite = np.isfinite(val).all(1)
    with np.errstate(invalid="ignore"):
        inside = val >= iso
    code = (inside << np.arange(dim + 1)).sum(1)
    k = np.tile(np.arange(nsimp), shape[0] * shape[1])
    zone = np.repeat(np.arange(NE), shape[1] * nsimp)
    _, rules = RULES[dim]
    nprim = np.array([[len(r) for r in rk] for rk in rules])
    count = np.where(finite, nprim[k, code], 0)
    start = np.cumsum(count) - count
    n = int(count.sum())
    edges = np.zeros((n, dim, 2), np.int32)
    t = np.zeros((n, dim))
    zo = np.zeros(n, np.int32)
    for kk in range(nsimp):
        for m in range(1 << (dim + 1)):
            rule = rules[kk][m]
            if not rule:
                continue
            sel = np.nonzero(finite & (k == kk) & (code == m))[0]
            if sel.size == 0:
                continue
            for j, prim in enumerate(rule):
                at = start[sel] + j
                zo[at] = zone[sel]
                for v, (a, b) in enumerate(prim):
                    edges[at, v, 0], edges[at, v, 1] = pts[sel, a], pts[sel, b]
                    s0, s1 = val[sel, a], val[sel, b]
                    t[at, v] = (iso - s0) / (s1 - s0)
    return edges, t, zo, int((~finite).sum())


def gather_reference(edges, t, field):
    """field (ncomp, NP) at the vertices: a + t (b - a), (ncomp, n, dim)"""
    field = np.asarray(field, np.float64)
    a, b = field[..., edges[..., 0]], field[..., edges[..., 1]]
    return a + t * (b - a)


def measure(points):
    """Sum of the areas (3D: points (3, n, 3) = component, primitive, vertex) or lengths (2D: (2, n, 2)) of the primitives"""
    P = np.moveaxis(np.asarray(points, np.float64), 0, -1)   # (n, vertex, component)
    if P.shape[-1] == 3:
        return float(0.5 * np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=1).sum())
    return float(np.linalg.norm(P[:, 1] - P[:, 0], axis=1).sum())


def box_lattice(zones, R1):
    """The lattice coordinates (dim, NP) of the undeformed unit box of `zones` equal zones per axis (x fastest)"""
    dim = len(zones)
    NE = int(np.prod(zones))
    e = np.arange(NE)
    zi = [e % zones[0], (e // zones[0]) % zones[1]] + ([e // (zones[0] * zones[1])] if dim == 3 else [])
    p = np.arange(R1 ** dim)
    ri = [p % R1, (p // R1) % R1] + ([p // (R1 * R1)] if dim == 3 else [])
    return np.stack([((zi[a][:, None] + ri[a][None, :] / (R1 - 1)) / zones[a]).reshape(-1) for a in range(dim)])
