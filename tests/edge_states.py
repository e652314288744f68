"""Edge states for the 2D/3D quadrature update (tests/test_gpu_qupdate_edges.py): the inputs helpers.deformed_state
never produces - uniform / planar compression and expansion (double and triple eigenvalues of the symmetric
gradient: a shock on an aligned mesh), rigid rotation and shear, a fluid at rest (hot, and cold: e = 0 as well),
negative energies (the fmax(0, e) clamp), still zones next to moving ones, a fluid at rest on a distorted mesh, an
inverted layer of zones (detJ < 0).

The affine-velocity states stay on the undeformed mesh on purpose: there Jpi = J J0^-1 = I, the length scale
h0 |Jpi d| / |d| does not depend on which eigenvector d of a repeated eigenvalue an implementation picks, and parity
with the oracle is well defined.  For the uniform ones the update has a closed form (closed_form below)."""
import numpy as np

from helpers import deformed_state

AFFINE = ("compress_iso", "expand_iso", "rotation", "shear")
STILL = ("still_hot", "still_cold")
DEFORMED = ("negative_e", "all_negative_e", "half_still", "still_deformed", "inverted_layer")


def state_names(dim):
    axes = "xyz"[:dim]
    return (AFFINE[:2] + tuple(f"compress_{a}" for a in axes) + tuple(f"expand_{a}" for a in axes)
            + AFFINE[2:] + STILL + DEFORMED)


def centre(prob):
    return np.array([0.5 * (b[0] + b[-1]) for b in prob.gbreaks])


def edge_state(prob, name):
    """the state vector [x | v | e] of the edge state `name` on `prob`"""
    dim, N, H1V = prob.dim, prob.N, prob.H1V
    S0 = prob.initial_state()[0]
    X = prob.node_coords()                       # (dim, N) initial positions
    c = centre(prob)
    if name in DEFORMED:
        S = deformed_state(prob, amp=0.0) if name == "inverted_layer" else deformed_state(prob)
        e = S[2 * H1V:]
        if name == "negative_e":
            e[::3] = -0.5
        elif name == "all_negative_e":
            e[:] = -1.0
        elif name == "still_deformed":
            # at rest on the distorted mesh: the gradient is exactly zero at every point (the `triple` branch, direction
            # e_x on both sides) while Jpi != I, so the direction shows - in dt, through the length scale of the viscosity
            S[H1V:2 * H1V] = 0.0
        elif name == "half_still":
            still = X[0] > c[0]
            for a in range(dim):
                S[H1V + a * N: H1V + (a + 1) * N][still] = 0.0
        else:
            bx = prob.gbreaks[0]
            k = (len(bx) - 1) // 2               # the middle x-layer of zones, reflected about its centre
            lo, hi = bx[k], bx[k + 1]
            x = S[:N]
            layer = (X[0] >= lo) & (X[0] <= hi)
            x[layer] = lo + hi - x[layer]
        return S
    S = S0.copy()
    v = np.zeros((dim, N))
    S[2 * H1V:] = 0.0 if name == "still_cold" else 1.0
    d = X - c[:, None]
    if name == "compress_iso":
        v = -d
    elif name == "expand_iso":
        v = d.copy()
    elif name.startswith("compress_") or name.startswith("expand_"):
        a = "xyz".index(name[-1])
        v[a] = -d[a] if name.startswith("compress_") else d[a]
    elif name == "rotation":
        v[0], v[1] = -d[1], d[0]
    elif name == "shear":
        v[0] = d[1]
    else:
        assert name in STILL, name
    S[H1V:2 * H1V] = v.reshape(-1)
    return S


# states whose de/dt is round-off on both sides by construction (see the de/dt scale in the test)
def de_is_roundoff(name, viscosity):
    """rotation: the symmetric gradient is round-off, so is stress : grad v.  Without viscosity the stress is -P I
    and stress : grad v = -P div v: round-off for shear as well."""
    return name == "rotation" or (name == "shear" and not viscosity)


CLOSED_FORM_STATES = ("compress_iso", "expand_iso", "compress_x", "expand_x", "still_hot")


def closed_form(prob, name, h0, cfl=0.5, rho=1.0, gamma=1.4, e=1.0):
    """(stressJinvT, dt) of the uniform states on the undeformed mesh of a Sedov configuration (rho0 = 1, gamma = 1.4,
    e = 1, unit rate), from the formulas of QUpdateBody alone (laghos_solver.cpp:1078-1160):
      stress = -P I + nu G,  P = (gamma - 1) rho e,  S = sqrt(gamma (gamma - 1) e),
      nu = 2 rho h0^2 |mu| + rho h0 S / 2 (1 - step(mu)),  mu the smallest eigenvalue of G (step = 0 for mu <= 0, 1 above 3e-12),
      stressJinvT[vd, gd] = stress[vd, gd] / w_gd * W_q * prod(w)   (J = diag(w): the zone's widths),
      dt = cfl / (S / h_min + 2.5 nu / (rho h_min^2)),  h_min = min(w over the mesh) / order_v."""
    dim, NE, NQ = prob.dim, prob.NE, prob.NQ
    P = (gamma - 1.0) * rho * e
    snd = np.sqrt(gamma * (gamma - 1.0) * e)
    G = {"compress_iso": -np.eye(dim), "expand_iso": np.eye(dim), "still_hot": np.zeros((dim, dim))}.get(name)
    if G is None:
        G = np.zeros((dim, dim))
        G[0, 0] = -1.0 if name == "compress_x" else 1.0
    mu = np.linalg.eigvalsh(G)[0]                 # diagonal with entries 0, +-1: exact
    nu = 2.0 * rho * h0 * h0 * abs(mu) + (0.5 * rho * h0 * snd if mu <= 0.0 else 0.0)
    stress = -P * np.eye(dim) + nu * G
    ei = prob.elem_index()
    w = np.stack([np.diff(prob.breaks[a])[ei[:, a]] for a in range(dim)], axis=1)    # (NE, dim)
    out = np.zeros((dim, dim, NE, NQ))
    for vd in range(dim):
        for gd in range(dim):
            out[vd, gd] = (stress[vd, gd] / w[:, gd] * np.prod(w, axis=1))[:, None] * prob.W[None, :]
    h_min = min(np.min(np.diff(b)) for b in prob.breaks) / prob.order_v
    dt = cfl / (snd / h_min + 2.5 * nu / (rho * h_min * h_min))
    return out.reshape(-1), dt
