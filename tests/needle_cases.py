"""Single deviating entries ("needles") for the checks that select a fast path from the caller's data, shared by
tests/test_needle_cases.py (CPU: the conditions the GPU tests rely on, on the oracle alone) and
tests/test_gpu_fast_path_checks.py (every check with one entry off).

The library takes a fast path where it FINDS a property in the data ("both properties are checked, never
assumed"): compact mass data D[q, e] = W[q] s_e (mass_rank1_k, one thread per zone, 256 zones per workgroup), one Jac0inv
per zone (jac0_compact_k, 64 zones per workgroup), mirror-symmetric 1-D tables and a symmetric tensor-product rule (host
loops of lgh_create), "the velocity of the state" (vec_differs_k: 16-byte loads, an odd tail, a scalar path) and "the
constant one" (not_all_ones_k).  Every other test has these checks pass everywhere, fail everywhere, or be bypassed by a
switch.  Here exactly one entry deviates, at the places a check would overlook first:

  per-zone checks   (zone, point) = (0, 0), (255, NQ - 1), (256, 0), (NE - 1, NQ - 1) and one in the middle on the
                    300-zone mesh (300 = 256 + 44 = 4 * 64 + 44: a ragged last workgroup of both kernels); first, middle
                    and last on the small meshes
  vectors           index 0, 1, n - 2, n - 1 and one in the middle

Meshes are shape_cases meshes (graded up to Q3Q2, equal above: shape_cases.solve_mesh): 10x6x5 for Q2Q1 and Q3Q2,
7x3x2 for Q4Q3, 17x1x1 for Q5Q4 and Q1Q0, 7x3 in 2D.

Wrappers are duck-typed like helpers.PermutedProblem (everything else comes from the base problem):
  OneCurvedZone   one zone of the initial mesh is not affine (its bubble node moved; at Q1Q0, or when asked, a vertex)
  SkewRule        an asymmetric quadrature rule under the same bases: asymmetric tables and / or asymmetric weights; the
                  zones stay affine and the mass data stays W[q] s_e
  TableNeedle     one entry of B, Bl or W changed; the operators are functions of the tables lgh_create is given, and the
                  oracle takes the same arrays"""
import numpy as np

import shape_cases as sc

BIG, MID, ROW, FLAT = (10, 6, 5), (7, 3, 2), (17, 1, 1), (7, 3)
# order -> shape of its 3D mesh
MESH_3D = {(2, 1): BIG, (3, 2): BIG, (4, 3): MID, (5, 4): ROW, (1, 0): ROW}
ORDERS_2D = [(2, 1), (3, 2)]

# the bars the GPU results are held to (tests/test_gpu_shapes_operators.py, test_gpu_k1.py)
BAR_STORED, BAR_COMPACT, BAR_QDATA = 1e-13, 2e-12, 1e-12
# what the checks admit (lgh_common.hpp: kMassRank1Tol, kJac0Tol) and the margins of the threshold cases
CHECK_TOL = 1e-12
SPREAD_BASE, SPREAD_BELOW, SPREAD_ABOVE = 1e-13, 2.5e-13, 4e-12
MASS_ABOVE, MASS_BELOW = 1.0 + 4e-12, 1.0 + 1e-13
MASS_SMALL = 1.0 + 3e-11   # seen at its own point only: the mean it moves leaves the zone's other points within half of CHECK_TOL
CURVE_ABOVE, CURVE_BELOW = 1e-10, 1e-14
# The far corner vertex of the LAST zone (a corner of the box: that zone's alone) moved by this much: the gradient of its
# basis function is largest at the nearest quadrature point - the zone's last - so Jac0inv deviates from the first point's
# by 1.27e-12 there and by at most 0.78e-12 (Q2Q1; 1 / 1.62 of it) or 0.73e-12 (Q3Q2; 1 / 1.76) at every other point: of
# all points only the last is beyond the 1e-12 the check admits (tests/test_needle_cases.py holds both margins)
CORNER_DELTA = {(2, 1): 1.45e-12, (3, 2): 1.1e-12}
CORNER_LAST, CORNER_OTHERS = 1.2e-12, 0.85e-12


def breaks(shape, mesh):
    """shape_cases.breaks; the graded 10x6x5 mesh by the same recipe without the demand that all zone volumes differ by
    2e-3 of themselves (300 products of 10, 6 and 5 widths within +-30 % cannot): widths mean * (1 + 0.25 u), u uniform in
    (-1, 1) from a fixed seed, rescaled to the axis length - hx != hy != hz in every zone, a few dozen distinct s_e"""
    if mesh == "equal" or int(np.prod(shape)) <= 64:
        return sc.breaks(shape, mesh)
    rng = np.random.default_rng([20241, int(np.prod(shape))])
    out = []
    for a, n in enumerate(shape):
        f = 1.0 + 0.25 * rng.uniform(-1.0, 1.0, n)
        b = np.concatenate([[0.0], np.cumsum(sc.AXIS_LENGTHS[a] * f / f.sum())])
        b[-1] = sc.AXIS_LENGTHS[a]
        out.append(b)
    return out


def problem(order, mesh=None, dim=3, problem=1):
    """the mesh of an order: graded up to Q3Q2, equal at Q4Q3 and Q5Q4 (shape_cases.solve_mesh: the energy CG of a whole
    right-hand side needs thousands of iterations on a graded mesh there)"""
    from oracle.fem import Problem
    mesh = mesh or sc.solve_mesh(order)
    shape = MESH_3D[order] if dim == 3 else FLAT
    prob = Problem(breaks=breaks(shape, mesh), order_v=order[0], order_e=order[1], problem=problem)
    assert tuple(prob.ne) == tuple(shape)
    return prob


def zone_points(NE, NQ):
    """(zone, point) of the needles of a per-zone check"""
    if NE > 256:
        return [(0, 0), (255, NQ - 1), (256, 0), (NE - 1, NQ - 1), (NE // 2 + 3, NQ // 2 + 1)]
    return [(0, 0), (NE // 2, NQ // 2 + 1), (NE - 1, NQ - 1)]


def curved_zones(NE):
    """zones of the OneCurvedZone cases: around the workgroup edge of jac0_compact_k where the mesh has one"""
    return [0, 63, 64, NE - 1] if NE > 64 else [0, NE // 2, NE - 1]


def vector_indices(n):
    return [0, 1, n // 2 + 1, n - 2, n - 1]


class OneCurvedZone:
    """`base` with ONE zone of the initial mesh not affine: the node with local index (1, 1, 1) of `zone` - interior to
    the zone for order_v >= 2, so no other zone sees it - is moved by delta * h * (1, 0.7, -0.5) (h: the zone's widths
    over the order).  At Q1Q0 there is no interior node: the zone's last vertex moves, and every zone that holds it
    deviates; vertex=True moves that vertex at any order.  `touched` lists the zones that hold the moved node."""
    AMOUNT = (1.0, 0.7, -0.5)

    def __init__(self, base, zone, delta, vertex=False):
        self.base, self.zone, self.delta = base, zone, delta
        S, self._rho_l2, self._gamma, self._rho0_q = base.initial_state()
        dim, D = base.dim, base.D1D
        hm = np.asarray(base.h1map).reshape(base.NE, base.ND)
        bubble = base.order_v >= 2 and not vertex
        local = sum(D ** a for a in range(dim)) if bubble else base.ND - 1
        self.node = int(hm[zone, local])
        self.touched = np.nonzero((hm == self.node).any(axis=1))[0]
        assert not bubble or list(self.touched) == [zone]
        ei = base.elem_index()[zone]
        X = S[:base.H1V].reshape(dim, base.N).copy()
        for a in range(dim):
            h = (base.breaks[a][ei[a] + 1] - base.breaks[a][ei[a]]) / base.order_v
            X[a, self.node] += delta * h * self.AMOUNT[a]
        self._S = np.concatenate([X.reshape(-1), S[base.H1V:]])

    def __getattr__(self, name):
        return getattr(self.base, name)

    def initial_state(self):
        # (rho0 = 1 in the problems this is used with: the values at the quadrature points stay)
        return self._S.copy(), self._rho_l2, self._gamma, self._rho0_q


def _tensor(w, dim):
    W = w
    for _ in range(dim - 1):
        W = np.multiply.outer(w, W)    # index [qz, qy, qx], as oracle.fem.Problem
    return W.reshape(-1)


class SkewRule:
    """`base` integrated with another rule under the same bases: the 1-D points x become x + skew_pts x (1 - x), the 1-D
    weights w (1 + skew_w (x - 1/2)).  H1 nodes, node coordinates and the Bernstein basis stay; B, G and Bl are the bases at
    the new points, W the tensor product of the new weights.  How well the rule integrates does not matter: both sides use
    the same tables."""

    def __init__(self, base, skew_pts, skew_w):
        from oracle.fem import bernstein_table, lagrange_tables
        self.base = base
        x = np.asarray(base.qpts)
        self.qpts = x + skew_pts * x * (1.0 - x)
        self.qwts = np.asarray(base.qwts) * (1.0 + skew_w * (x - 0.5))
        assert np.all(self.qwts > 0) and np.all(np.diff(self.qpts) > 0) and 0 < self.qpts[0] and self.qpts[-1] < 1
        self.B, self.G = lagrange_tables(base.gll, self.qpts)
        self.Bl = bernstein_table(base.order_e, self.qpts)
        self.W = _tensor(self.qwts, base.dim)

    def __getattr__(self, name):
        return getattr(self.base, name)

    def initial_state(self):
        S, rho_l2, gamma, _ = self.base.initial_state()
        rho0_q = self.base.rho0(self.base.elem_points(self.qpts)).reshape(-1)    # the coefficient at the points of THIS rule
        return S, rho_l2, gamma, rho0_q


class TableNeedle:
    """`base` with one entry of a table changed: which = "B" or "Bl" (index into the array lgh_create is given,
    [q + Q1D d]) or "W" (index q); the entry becomes entry * scale + eps."""

    def __init__(self, base, which, index, eps=0.0, scale=1.0):
        assert which in ("B", "Bl", "W")
        self.base, self.which, self.index = base, which, index
        t = np.array(getattr(base, which), dtype=np.float64, copy=True)
        if which == "W":
            t[index] = t[index] * scale + eps
        else:
            Q = base.Q1D
            t[index % Q, index // Q] = t[index % Q, index // Q] * scale + eps
        setattr(self, which, t)

    def __getattr__(self, name):
        return getattr(self.base, name)


class WithTables:
    """`base` with whole tables replaced (B, G, Bl, W as keywords): what a fast path that misjudged the caller's tables
    would compute with - the oracle emulates the wrong path through it"""

    def __init__(self, base, **tables):
        assert set(tables) <= {"B", "G", "Bl", "W"}
        self.base = base
        for k, v in tables.items():
            setattr(self, k, np.array(v, dtype=np.float64, copy=True))

    def __getattr__(self, name):
        return getattr(self.base, name)


def table_indices(n):
    """first, middle, last index of a table of n entries (n is even for every rule here: no entry is its own mirror image)"""
    assert n % 2 == 0
    return [0, n // 2 + 1, n - 1]


# ---- what a check looks at, on host arrays ---------------------------------------------------------------------------
def mass_spread(D, W, NE):
    """per zone: max_q |D[q] - W[q] s| / |D[q]| with s = mean_q D[q] / W[q] - the quantity mass_rank1_k holds against
    kMassRank1Tol - and the compact table W[q] s the fast path would read instead"""
    D = np.asarray(D, dtype=np.float64).reshape(NE, -1)
    with np.errstate(all="ignore"):
        s = (D / W).mean(axis=1)
        compact = W[None, :] * s[:, None]
        return (np.abs(D - compact) / np.abs(D)).max(axis=1), compact.reshape(-1)


def mass_threshold_position(D0, W, NE):
    """The entry of the threshold needles: the one that lies furthest ABOVE its zone's mean of D / W.  A factor 1 + t on
    one entry of a zone of NQ points moves that entry t (1 - 1 / NQ) away from the new mean; with the entry's own
    rounding on top the spread of the "just above" needle reaches t = 4e-12 only where that rounding has the same sign
    and at least t / NQ (1.9e-14 at Q3Q2; at Q2Q1, NQ = 64, no entry of the mesh has the 6.3e-14 it would take)."""
    r = np.asarray(D0).reshape(NE, -1) / W
    dev = (r - r.mean(axis=1, keepdims=True)) / r
    return int(np.argmax(dev))


def jac0_spread(J, NE, NQ, n2):
    """per zone: max |J(q) - J(0)| / max |J(0)| - what jac0_compact_k holds against kJac0Tol - and the array with every
    point's matrix replaced by the zone's first, as the compact form reads it"""
    J = np.asarray(J, dtype=np.float64).reshape(NE, NQ, n2)
    first = np.repeat(J[:, :1, :], NQ, axis=1)
    return np.abs(J - first).max(axis=(1, 2)) / np.abs(J[:, 0, :]).max(axis=1), first.reshape(-1)


def mirrored(T, keep):
    """the (Q, n) table a kernel that keeps half of it in registers would use: the half `keep` (0: entries of the first
    half of the flat array, 1: of the second) and its mirror image"""
    flat = np.asarray(T, dtype=np.float64).T.reshape(-1).copy()
    n = flat.size
    if keep == 0:
        flat[n - n // 2:] = flat[:n // 2][::-1]
    else:
        flat[:n // 2] = flat[n - n // 2:][::-1]
    return np.ascontiguousarray(flat.reshape(np.asarray(T).shape[::-1]).T)


def rebuilt_weights(W, Q, dim):
    """the weights as lgh_create rebuilds them when it takes the rule for a symmetric tensor product: w[i] = W[i, 0, 0] /
    w[0]^(dim - 1), w[0] = W[0]^(1 / dim), the second half mirrored from the first"""
    W = np.asarray(W, dtype=np.float64)
    w0 = W[0] ** (1.0 / dim)
    w = W[:Q] / w0 ** (dim - 1)
    for i in range(Q // 2):
        w[Q - 1 - i] = w[i]
    return _tensor(w, dim)


def tile_condition(T, w):
    """condition number of the 1-D mass tile T^T diag(w) T"""
    T = np.asarray(T, dtype=np.float64)
    return float(np.linalg.cond(T.T @ (np.asarray(w)[:, None] * T)))


def jac0_point_spread(J, NE, NQ, n2):
    """(NE, NQ): max_k |J(q)[k] - J(0)[k]| / max_k |J(0)[k]| - what jac0_compact_k compares with kJac0Tol point by point"""
    J = np.asarray(J, dtype=np.float64).reshape(NE, NQ, n2)
    return np.abs(J - J[:, :1, :]).max(axis=2) / np.abs(J[:, 0, :]).max(axis=1)[:, None]
