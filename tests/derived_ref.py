"""numpy restatement of the derived lattice fields (lgh_sample_derived) for the tests: the derivative table of the H1
basis from the Lagrange formula on lattice_ref.gll_nodes, J = dx/dxi and V = dv/dxi by dense einsums over the element ->
node map, L = V inv(J), and the per-point error scales of DESIGN.md §7f.  Shares no code with the library.  Every
routine works in the dtype it is given (np.float64, or np.longdouble for the reference's own error)."""
import numpy as np

from lattice_ref import bernstein_table, gll_nodes

TOL = 1e-13   # the figure of tests/test_gpu_sample.py for sums of at most D1D^dim <= 125 products


def lagrange_grad_table(nodes, pts):
    """G[r, d] = l_d'(pts[r]) = sum_{k != d} 1 / (x_d - x_k) prod_{m != d, k} (x - x_m) / (x_d - x_m)"""
    G = np.zeros((len(pts), len(nodes)), dtype=np.result_type(nodes, pts))
    for d, xd in enumerate(nodes):
        for k, xk in enumerate(nodes):
            if k == d:
                continue
            term = np.ones(len(pts), dtype=G.dtype) / (xd - xk)
            for m, xm in enumerate(nodes):
                if m != d and m != k:
                    term = term * (pts - xm) / (xd - xm)
            G[:, d] += term
    return G


def lattice_tables3(order_v, order_e, R, dtype=np.float64):
    """(B_h1, G_h1, B_l2) at r/R, indexed [r, d]"""
    pts = np.arange(R + 1, dtype=dtype) / dtype(R)
    nodes = gll_nodes(order_v + 1).astype(dtype)   # (the float64 nodes in both precisions: the same basis)
    return _lagrange(nodes, pts), lagrange_grad_table(nodes, pts), bernstein_table(order_e, pts)


def _lagrange(nodes, pts):
    B = np.ones((len(pts), len(nodes)), dtype=pts.dtype)
    for d, xd in enumerate(nodes):
        for m, xm in enumerate(nodes):
            if m != d:
                B[:, d] = B[:, d] * (pts - xm) / (xd - xm)
    return B


def _contract(U, T, dim):
    """U[e, (dz, dy,) dx], T = the table per axis (x, y, z) -> [e * NPZ + rx + R1 (ry + R1 rz)]"""
    if dim == 1:
        out = np.einsum("ex,ix->ei", U, T[0])
    elif dim == 2:
        out = np.einsum("eyx,jy,ix->eji", U, T[1], T[0])
    else:
        out = np.einsum("ezyx,kz,jy,ix->ekji", U, T[2], T[1], T[0])
    return out.reshape(-1)


def _jacobian(F, hm, B, G, dim):
    """[pt, i, j] = d F_i / d xi_j of the dim nodal fields F (dim, N)"""
    return np.stack([np.stack([_contract(F[i][hm], [G if a == j else B for a in range(dim)], dim) for j in range(dim)], axis=-1)
                     for i in range(dim)], axis=1)


def _inverse(J):
    """inv of [pt, dim, dim]: numpy's in float64, the adjugate over the determinant where numpy has no LAPACK (longdouble)"""
    if J.dtype == np.float64:
        return np.linalg.inv(J)
    n = J.shape[-1]
    if n == 1:
        return 1 / J
    if n == 2:
        det = J[:, 0, 0] * J[:, 1, 1] - J[:, 0, 1] * J[:, 1, 0]
        A = np.stack([np.stack([J[:, 1, 1], -J[:, 0, 1]], -1), np.stack([-J[:, 1, 0], J[:, 0, 0]], -1)], 1)
        return A / det[:, None, None]
    A = np.empty_like(J)
    for i in range(3):
        for j in range(3):
            a, b = (j + 1) % 3, (j + 2) % 3
            c, d = (i + 1) % 3, (i + 2) % 3
            A[:, i, j] = J[:, a, c] * J[:, b, d] - J[:, a, d] * J[:, b, c]
    det = (J[:, 0, :] * A[:, :, 0]).sum(-1)
    return A / det[:, None, None]


def _det(J):
    n = J.shape[-1]
    if n == 1:
        return J[:, 0, 0]
    if n == 2:
        return J[:, 0, 0] * J[:, 1, 1] - J[:, 0, 1] * J[:, 1, 0]
    return (J[:, 0, 0] * (J[:, 1, 1] * J[:, 2, 2] - J[:, 1, 2] * J[:, 2, 1]) - J[:, 0, 1] * (J[:, 1, 0] * J[:, 2, 2] - J[:, 1, 2] * J[:, 2, 0])
            + J[:, 0, 2] * (J[:, 1, 0] * J[:, 2, 1] - J[:, 1, 1] * J[:, 2, 0]))


def _fro(M):
    return np.sqrt((M.reshape(M.shape[0], -1) ** 2).sum(-1))


def derived_reference(dim, NE, N, D1D, L1D, h1map, S, gamma, Bh, Gh, Bl):
    """dict in the layouts of lgh_sample_derived: detj, div_v, sound_speed, e (NP), grad_v (dim^2, NP), vorticity (NP in 2D,
    (3, NP) in 3D, absent in 1D), zones in the order of h1map; and the error scales per point (to be multiplied by TOL):
    bound_L   = (|A_V|_F + |L|_F |A_J|_F) |J^-1|_F + kappa_F(J) |L|_F     for |L_gpu - L|_F
    bound_det = |A_J|_F |J^-1|_F |det J|                                   for |detJ_gpu - det J|
    with A_J, A_V the contractions of J, V done with the absolute values of tables and dofs.  Works in the dtype of Bh."""
    dt = Bh.dtype
    S, gamma = np.asarray(S).astype(dt), np.asarray(gamma).astype(dt)
    hm = np.asarray(h1map).reshape(NE, *([D1D] * dim))
    H1V = dim * N
    X, Vn = S[:H1V].reshape(dim, N), S[H1V:2 * H1V].reshape(dim, N)
    J, V = _jacobian(X, hm, Bh, Gh, dim), _jacobian(Vn, hm, Bh, Gh, dim)
    AJ, AV = _jacobian(np.abs(X), hm, np.abs(Bh), np.abs(Gh), dim), _jacobian(np.abs(Vn), hm, np.abs(Bh), np.abs(Gh), dim)
    Jinv = _inverse(J)
    L = np.einsum("pik,pkj->pij", V, Jinv)
    NP = L.shape[0]
    out = dict(detj=_det(J), grad_v=L.reshape(NP, dim * dim).T.copy(), div_v=np.einsum("pii->p", L))
    if dim == 2:
        out["vorticity"] = L[:, 1, 0] - L[:, 0, 1]
    elif dim == 3:
        out["vorticity"] = np.stack([L[:, 2, 1] - L[:, 1, 2], L[:, 0, 2] - L[:, 2, 0], L[:, 1, 0] - L[:, 0, 1]])
    e = _contract(S[2 * H1V:].reshape(NE, *([L1D] * dim)), [Bl] * dim, dim)
    g = np.repeat(gamma, NP // NE)
    out["e"] = e
    out["sound_speed"] = np.sqrt((g * (g - 1)) * np.maximum(e, 0))
    nL, nJi = _fro(L), _fro(Jinv)
    out["bound_L"] = (_fro(AV) + nL * _fro(AJ)) * nJi + _fro(J) * nJi * nL
    out["bound_det"] = _fro(AJ) * nJi * np.abs(out["detj"])
    return out


def curved_state(zones, ok, ot):
    """The discretisation and the random state on a curved mesh of tests/test_gpu_sample.py's Case (lexicographic numbering), made
    without a GPU and with the same seeds: dict dim, NE, N, D, L, h1map, S, gamma, x (dim, N) node positions."""
    from oracle.fem import Problem
    dim = len(zones)
    p = Problem(breaks=[np.linspace(0.0, 1.0, n + 1) for n in zones], order_v=ok, order_e=ot, problem=1)
    x0 = p.initial_state()[0][:p.H1V]
    NE, N, H1V, NL = int(np.prod(zones)), p.N, dim * p.N, (ot + 1) ** dim
    rng = np.random.default_rng(1000 * dim + 10 * ok + NE)
    hmin = 1.0 / (max(zones) * ok)
    S = np.concatenate([x0 + 0.2 * hmin * rng.uniform(-1, 1, H1V), rng.uniform(-1, 1, H1V), rng.uniform(-0.5, 1.0, NE * NL)])
    rng.uniform(0.5, 2.0, NE * NL)   # (the density dofs of Case)
    gamma = rng.uniform(1.2, 1.8, NE)
    return dict(dim=dim, NE=NE, N=N, D=ok + 1, L=ot + 1, ok=ok, ot=ot, h1map=np.asarray(p.h1map).reshape(-1), S=S, gamma=gamma)


def affine_velocity(S, dim, N, A, b):
    """S with v = A x + b at the nodes"""
    S = S.copy()
    H1V = dim * N
    X = S[:H1V].reshape(dim, N)
    S[H1V:2 * H1V] = (np.asarray(A) @ X + np.asarray(b)[:, None]).reshape(-1)
    return S
