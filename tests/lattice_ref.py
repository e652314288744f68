"""numpy restatement of the visualisation sampling for the tests: the 1-D bases at the lattice abscissae r/R written
from their formulas (Gauss-Lobatto points from numpy.polynomial.legendre), and the lattice values of a state by a
dense einsum over the element -> node map.  Shares no code with the library."""
from math import comb

import numpy as np


def gll_nodes(n):
    """n Gauss-Lobatto points on [0, 1]: the ends and the roots of P'_{n-1}"""
    inner = np.polynomial.legendre.Legendre.basis(n - 1).deriv().roots() if n > 2 else np.zeros(0)
    return 0.5 * (1.0 + np.concatenate([[-1.0], np.sort(inner.real), [1.0]]))


def lagrange_table(nodes, pts):
    """B[r, d] = l_d(pts[r]), Lagrange basis on `nodes`"""
    B = np.ones((len(pts), len(nodes)))
    for d, xd in enumerate(nodes):
        for m, xm in enumerate(nodes):
            if m != d:
                B[:, d] *= (pts - xm) / (xd - xm)
    return B


def bernstein_table(p, pts):
    """B[r, l] = C(p, l) x^l (1 - x)^(p - l)"""
    return np.stack([comb(p, l) * pts ** l * (1.0 - pts) ** (p - l) for l in range(p + 1)], axis=1)


def lattice_tables(order_v, order_e, R):
    pts = np.arange(R + 1) / R
    return lagrange_table(gll_nodes(order_v + 1), pts), bernstein_table(order_e, pts)


def _contract(U, T, dim):
    """U[e, (dz, dy,) dx] -> [e, (rz, ry,) rx] flattened per zone: pt = rx + R1 (ry + R1 rz)"""
    if dim == 1:
        out = np.einsum("ex,ix->ei", U, T)
    elif dim == 2:
        out = np.einsum("eyx,jy,ix->eji", U, T, T)
    else:
        out = np.einsum("ezyx,kz,jy,ix->ekji", U, T, T, T)
    return out.reshape(-1)


def sample_reference(dim, NE, N, D1D, L1D, h1map, S, rho_l2, gamma, Bh, Bl):
    """dict x, v (dim, NP), e, rho, p (NP): the lattice values lgh_sample_fields is to produce, zones in the order of
    h1map; p = (gamma_z - 1) rho max(e, 0) from the sampled factors"""
    hm = np.asarray(h1map).reshape(NE, *([D1D] * dim))
    R1 = Bh.shape[0]
    H1V = dim * N
    out = {}
    for name, off in (("x", 0), ("v", H1V)):
        out[name] = np.stack([_contract(S[off + c * N: off + (c + 1) * N][hm], Bh, dim) for c in range(dim)])
    shp = (NE, *([L1D] * dim))
    out["e"] = _contract(S[2 * H1V:].reshape(shp), Bl, dim)
    out["rho"] = _contract(np.asarray(rho_l2).reshape(shp), Bl, dim)
    out["p"] = (np.repeat(np.asarray(gamma), R1 ** dim) - 1.0) * out["rho"] * np.maximum(out["e"], 0.0)
    return out
