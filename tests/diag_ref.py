"""numpy restatement of lgh_diagnostics for the tests: the point values by a dense einsum of the test's own tables over the
element -> node map (as tests/lattice_ref.py does for the sampling), then the 17 zone figures and the 20 global ones of
include/laghos_hip.h.  Shares no code with the library.  m_q (rho0DetJ0w) is an input: the tests read it back from the
context, where existing tests hold it to the oracle.

Beside the figures it returns what the bounds of the tests are made of:
  abs_zone / abs_glob   sum_q |term| of each of the 7 sums (mass, volume, ie, ke, px, py, pz), per zone and over the mesh;
  kappa                 the condition of detJ as data formed from J = sum G x (kappa = max sum|G x| / |J|).
                        For a dim x dim Jacobian a rounding error of eps A_cj in entry J_cj, A_cj = sum_d |G| |x_d| the sum
                        of the absolute terms, moves detJ by |cof_cj| eps A_cj, so
                            kappa = max_q  sum_cj |cof_cj| A_cj / |detJ_q|
                        which is sum|G x| / |J| in 1D."""
import numpy as np

SUMS = (0, 1, 2, 3, 4, 5, 6)
MINS = (7, 8, 10)
MAXS = (9, 11, 12, 13)
COUNTS = (14, 15, 16)
NAMES = ("mass", "volume", "ie", "ke", "px", "py", "pz", "detj_min", "rho_min", "rho_max", "e_min", "e_max", "p_max", "v_max",
         "n_inverted", "n_negative_e", "n_nonfinite")


def _interp(U, tabs, dim):
    """U[e, (dz, dy,) dx] with the table of every axis (x first), T[q, d] -> values [e, q], q = qx + Q (qy + Q qz)"""
    if dim == 1:
        out = np.einsum("ex,ix->ei", U, tabs[0])
    elif dim == 2:
        out = np.einsum("eyx,jy,ix->eji", U, tabs[1], tabs[0])
    else:
        out = np.einsum("ezyx,kz,jy,ix->ekji", U, tabs[2], tabs[1], tabs[0])
    return out.reshape(U.shape[0], -1)


def _det_and_cof(J, dim):
    """J[e, q, c, j] -> (det [e, q], |cofactors| [e, q, c, j])"""
    if dim == 1:
        return J[..., 0, 0], np.ones_like(J)
    if dim == 2:
        det = J[..., 0, 0] * J[..., 1, 1] - J[..., 0, 1] * J[..., 1, 0]
        cof = np.empty_like(J)
        cof[..., 0, 0], cof[..., 0, 1], cof[..., 1, 0], cof[..., 1, 1] = J[..., 1, 1], J[..., 1, 0], J[..., 0, 1], J[..., 0, 0]
        return det, np.abs(cof)
    cof = np.empty_like(J)
    for c in range(3):
        for j in range(3):
            a, b = [k for k in range(3) if k != c], [k for k in range(3) if k != j]
            cof[..., c, j] = J[..., a[0], b[0]] * J[..., a[1], b[1]] - J[..., a[0], b[1]] * J[..., a[1], b[0]]
    det = J[..., 0, 0] * cof[..., 0, 0] - J[..., 0, 1] * cof[..., 0, 1] + J[..., 0, 2] * cof[..., 0, 2]
    return det, np.abs(cof)


def point_values(dim, NE, N, D1D, L1D, h1map, S, B, G, Bl):
    """dict detJ, e [NE, NQ], v [dim, NE, NQ], kappa"""
    hm = np.asarray(h1map).reshape(NE, *([D1D] * dim))
    H1V = dim * N
    Q = B.shape[0]
    NQ = Q ** dim
    J, A = np.empty((NE, NQ, dim, dim)), np.empty((NE, NQ, dim, dim))
    for c in range(dim):
        xc = S[c * N:(c + 1) * N][hm]
        # offsets from the zone's first node: the rows of G sum to zero, so the gradient is the same and is formed without the
        # cancellation of O(1) coordinates in O(h) differences (kappa below stays the rule's, from the coordinates themselves)
        xa = np.abs(xc)
        xc = xc - xc.reshape(NE, -1)[:, 0].reshape(NE, *([1] * dim))
        for j in range(dim):
            tabs = [G if a == j else B for a in range(dim)]
            J[:, :, c, j] = _interp(xc, tabs, dim)
            A[:, :, c, j] = _interp(xa, [np.abs(t) for t in tabs], dim)
    det, cof = _det_and_cof(J, dim)
    with np.errstate(all="ignore"):
        kappa = float(np.nanmax((cof * A).sum(axis=(2, 3)) / np.abs(det)))
    v = np.stack([_interp(S[H1V + c * N:H1V + (c + 1) * N][hm], [B] * dim, dim) for c in range(dim)])
    e = _interp(S[2 * H1V:].reshape(NE, *([L1D] * dim)), [Bl] * dim, dim)
    return dict(detJ=det, e=e, v=v, kappa=kappa)


def diag_reference(dim, NE, N, D1D, L1D, h1map, S, m, gamma, W, B, G, Bl):
    """dict zone [17, NE], glob [20], abs_zone [7, NE], abs_glob [7], kappa, detJ, e [NE, NQ]"""
    pv = point_values(dim, NE, N, D1D, L1D, h1map, S, B, G, Bl)
    det, e, v = pv["detJ"], pv["e"], pv["v"]
    NQ = det.shape[1]
    m = np.asarray(m).reshape(NE, NQ)
    w = np.asarray(W).reshape(1, NQ)
    gm1 = np.asarray(gamma).reshape(NE, 1) - 1.0
    with np.errstate(all="ignore"):
        v2 = (v * v).sum(axis=0)
        finite = np.isfinite(det) & np.isfinite(e) & np.isfinite(v).all(axis=0)
        inverted = det <= 0.0
        good = finite & ~inverted
        rho = m / (w * det)
        p = gm1 * rho * np.maximum(e, 0.0)
        terms = [m, w * det, m * e, 0.5 * m * v2] + [m * v[c] for c in range(dim)] + [np.zeros_like(m)] * (3 - dim)
    zone, azone = np.empty((17, NE)), np.empty((7, NE))
    for k, t in enumerate(terms):
        zone[k], azone[k] = t.sum(axis=1), np.abs(t).sum(axis=1)

    def ext(a, mask, lo):
        return np.where(mask, a, np.inf).min(axis=1) if lo else np.where(mask, a, -np.inf).max(axis=1)
    zone[7] = ext(det, finite, True)
    zone[8], zone[9] = ext(rho, good, True), ext(rho, good, False)
    zone[10], zone[11] = ext(e, finite, True), ext(e, finite, False)
    zone[12] = ext(p, good, False)
    zone[13] = ext(np.sqrt(v2), finite, False)
    zone[14], zone[15], zone[16] = inverted.sum(axis=1), (e < 0.0).sum(axis=1), (~finite).sum(axis=1)
    glob = np.zeros(20)
    for k in SUMS + COUNTS:
        glob[k] = zone[k].sum()
    for k in MINS:
        glob[k] = zone[k].min()
    for k in MAXS:
        glob[k] = zone[k].max()
    glob[17] = int(np.argmin(zone[7]))        # (the first zone that holds the minimum)
    return dict(zone=zone, glob=glob, abs_zone=azone, abs_glob=azone.sum(axis=1), kappa=pv["kappa"], detJ=det, e=e)
