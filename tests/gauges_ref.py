"""numpy restatement of the gauges (lgh_gauges_*, the driver's `-gauges`) for the tests: the 1-D bases at an arbitrary
reference coordinate from their formulas (lattice_ref.gll_nodes, lattice_ref.bernstein_table, derived_ref._lagrange,
derived_ref.lagrange_grad_table), the point values by dense einsums per gauge over the element -> node map, as
derived_ref.derived_reference forms them on a lattice, and the location of a point in the initial tensor grid.  Shares no code
with the library.  Every routine works in the dtype of the tables it is given (np.float64, or np.longdouble for the
reference's own error).

A gauge is (zone, xi): rows of GAUGE_COLS,
    x, v      the H1 fields at xi                     e      the L2 field at xi
    detj      det(dx/dxi)                             div_v  tr((dv/dxi) J^-1)
    rho       m_g / detj,  m_g = rho0(xi) detJ0(xi)   p      (gamma_z - 1) rho max(e, 0)
    cs        sqrt(gamma_z (gamma_z - 1) max(e, 0))
with the components of x and v beyond the dimension 0."""
import numpy as np

from derived_ref import TOL, _det, _fro, _inverse, _lagrange, lagrange_grad_table
from lattice_ref import bernstein_table, gll_nodes

GAUGE_COLS = ("x", "y", "z", "vx", "vy", "vz", "rho", "e", "p", "cs", "detj", "div_v")


def tables_at(order_v, order_e, xi, dtype=np.float64):
    """xi (n, dim) -> Bh, Gh (n, dim, D1D) and Bl (n, dim, L1D): [g, a, d] = basis function d at xi[g, a]"""
    xi = np.asarray(xi, dtype=dtype)
    n, dim = xi.shape
    nodes = gll_nodes(order_v + 1).astype(dtype)   # (the float64 nodes in both precisions: the same basis)
    pts = xi.reshape(-1)
    shape = lambda T: T.reshape(n, dim, -1)
    return shape(_lagrange(nodes, pts)), shape(lagrange_grad_table(nodes, pts)), shape(bernstein_table(order_e, pts))


def _at(U, T):
    """U[(dz, dy,) dx] contracted with the 1-D rows T = [x, y, z]"""
    dim = U.ndim
    if dim == 1:
        return np.einsum("x,x->", U, T[0])
    if dim == 2:
        return np.einsum("yx,y,x->", U, T[1], T[0])
    return np.einsum("zyx,z,y,x->", U, T[2], T[1], T[0])


def _point(F, nodes, B, G):
    """values (dim,) and derivatives [i, j] = dF_i/dxi_j of the nodal fields F (dim, N) at one gauge (nodes: the zone's map)"""
    dim = F.shape[0]
    val = np.array([_at(F[i][nodes], [B[a] for a in range(dim)]) for i in range(dim)], dtype=B.dtype)
    jac = np.array([[_at(F[i][nodes], [G[a] if a == j else B[a] for a in range(dim)]) for j in range(dim)] for i in range(dim)], dtype=B.dtype)
    return val, jac


def gauges_mass_reference(dim, NE, N, D1D, L1D, h1map, x0, rho0_l2, zone, Bh, Gh, Bl):
    """m_g = rho0(xi_g) detJ0(xi_g), and rho0(xi_g)"""
    dt = Bh.dtype
    hm = np.asarray(h1map).reshape(NE, *([D1D] * dim))
    X = np.asarray(x0).astype(dt).reshape(dim, N)
    R = np.asarray(rho0_l2).astype(dt).reshape(NE, *([L1D] * dim))
    m, r0 = np.zeros(len(zone), dtype=dt), np.zeros(len(zone), dtype=dt)
    for g, z in enumerate(zone):
        _, J = _point(X, hm[z], Bh[g], Gh[g])
        r0[g] = _at(R[z], [Bl[g][a] for a in range(dim)])
        m[g] = r0[g] * _det(J[None])[0]
    return m, r0


def gauges_reference(dim, NE, N, D1D, L1D, h1map, S, gamma, zone, Bh, Gh, Bl, mass):
    """dict rows (n, 12) by GAUGE_COLS and, per gauge, the error scales of DESIGN.md §7f (to be multiplied by TOL):
    bound_det for |detj - ref| and bound_L for the Frobenius error of L = (dv/dxi) J^-1 (|div_v - ref| <= dim TOL bound_L),
    as derived_ref.derived_reference states them."""
    dt = Bh.dtype
    S, gamma, mass = np.asarray(S).astype(dt), np.asarray(gamma).astype(dt), np.asarray(mass).astype(dt)
    hm = np.asarray(h1map).reshape(NE, *([D1D] * dim))
    H1V = dim * N
    X, V = S[:H1V].reshape(dim, N), S[H1V:2 * H1V].reshape(dim, N)
    E = S[2 * H1V:].reshape(NE, *([L1D] * dim))
    n = len(zone)
    rows = np.zeros((n, len(GAUGE_COLS)), dtype=dt)
    bound_det, bound_L = np.zeros(n, dtype=dt), np.zeros(n, dtype=dt)
    for g, z in enumerate(zone):
        x, J = _point(X, hm[z], Bh[g], Gh[g])
        v, dV = _point(V, hm[z], Bh[g], Gh[g])
        _, AJ = _point(np.abs(X), hm[z], np.abs(Bh[g]), np.abs(Gh[g]))
        _, AV = _point(np.abs(V), hm[z], np.abs(Bh[g]), np.abs(Gh[g]))
        e = _at(E[z], [Bl[g][a] for a in range(dim)])
        det = _det(J[None])[0]
        Jinv = _inverse(J[None])[0]
        L = dV @ Jinv
        rho = mass[g] / det
        gz = gamma[z]
        rows[g, :dim], rows[g, 3:3 + dim] = x, v
        rows[g, 6:] = [rho, e, (gz - 1) * rho * max(e, 0), np.sqrt((gz * (gz - 1)) * max(e, 0)), det, np.trace(L)]
        nL, nJi = _fro(L[None])[0], _fro(Jinv[None])[0]
        bound_det[g] = _fro(AJ[None])[0] * nJi * abs(det)
        bound_L[g] = (_fro(AV[None])[0] + nL * _fro(AJ[None])[0]) * nJi + _fro(J[None])[0] * nJi * nL
    return dict(rows=rows, bound_det=bound_det, bound_L=bound_L)


def locate_initial(breaks, X):
    """The location rule of a gauge in the initial mesh: breaks = the break points per axis of the tensor grid,
    X the position.  Per axis the interval is [brk_i, brk_{i+1}), the last one closed; xi = (X - brk_i) / (brk_{i+1} - brk_i).
    -> (zone index per axis, xi per axis); ValueError for a point outside the mesh or not finite."""
    ijk, xi = [], []
    for a, brk in enumerate(breaks):
        brk = np.asarray(brk, dtype=np.float64)
        x = float(X[a])
        if not np.isfinite(x) or x < brk[0] or x > brk[-1]:
            raise ValueError(f"coordinate {a} = {x} is outside [{brk[0]}, {brk[-1]}]")
        i = min(int(np.searchsorted(brk, x, side="right")) - 1, len(brk) - 2)
        ijk.append(i)
        xi.append((x - brk[i]) / (brk[i + 1] - brk[i]))
    return ijk, xi


HEADER = "cycle t gauge x y z vx vy vz rho e p cs detj div_v"


def _num(v):
    return "nan" if np.isnan(v) else "%.17g" % v


def gauges_text(cycle, t, rows):
    """The lines of one sample in <basename>_gauges.csv under HEADER, one per gauge: cycle and gauge as integers, the rest with %.17g
    (inf, -inf, nan as they come)."""
    return "".join(" ".join([str(int(cycle)), _num(t), str(g)] + [_num(v) for v in r]) + "\n" for g, r in enumerate(np.asarray(rows).reshape(-1, 12)))
