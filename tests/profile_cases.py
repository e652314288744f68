"""The inputs of the profile tests, without a GPU: the states of tests/test_gpu_diagnostics.py's `Case` recipe (curved mesh
x0 + 0.2 h rng, random v, e, rho0_q, gamma - the same generator calls in the same order, so the same numbers; the GPU test
checks that against the Case it builds) and the specs every case is binned under.  tests/test_profile_ref.py holds the specs
to `undecided == 0` on the CPU, which is what lets the GPU tests demand exact counts."""
import numpy as np

ZONES = {"1D-1": (1,), "1D-3": (3,), "1D-257": (257,), "2D-3x2": (3, 2), "3D-3x2x2": (3, 2, 2), "3D-5x5x3": (5, 5, 3),
         "3D-2x2x1": (2, 2, 1)}
ORDERS = [(1, 0), (2, 1), (3, 2)]
CASES = [(z, o) for z in list(ZONES)[:6] for o in ORDERS] + [("2D-3x2", (4, 3)), ("3D-2x2x1", (5, 4))]
IDS = [f"{z}-Q{o[0]}Q{o[1]}" for z, o in CASES]


def case_data(zones, ok, ot):
    """what Case(zones, ok, ot) of tests/test_gpu_diagnostics.py holds, as a dict, without a context"""
    from oracle.fem import Problem
    dim = len(zones)
    p = Problem(breaks=[np.linspace(0.0, 1.0, n + 1) for n in zones], order_v=ok, order_e=ot, problem=1)
    x0 = p.initial_state()[0][:p.H1V]
    NE, N, D, L = int(np.prod(zones)), p.N, ok + 1, ot + 1
    Q = p.B.shape[0]
    H1V, NL, NQ = dim * N, L ** dim, Q ** dim
    rng = np.random.default_rng(1000 * dim + 10 * ok + NE)
    hmin = 1.0 / (max(zones) * ok)
    S = np.concatenate([x0 + 0.2 * hmin * rng.uniform(-1, 1, H1V), rng.uniform(-1, 1, H1V), rng.uniform(-0.5, 1.0, NE * NL)])
    rho0_l2 = rng.uniform(0.5, 2.0, NE * NL)
    rho0_q = rng.uniform(0.5, 2.0, NE * NQ)
    gamma = rng.uniform(1.2, 1.8, NE)
    return dict(dim=dim, NE=NE, N=N, D=D, L=L, Q=Q, NQ=NQ, ND=D ** dim, h1map=np.asarray(p.h1map).reshape(-1), W=np.asarray(p.W), B=p.B, G=p.G,
                Bl=p.Bl, S=S, x0=x0, rho0_l2=rho0_l2, rho0_q=rho0_q, gamma=gamma)


def specs(dim):
    """(name, axis, nbins, lo, hi, origin): every axis of the dimension with 7 bins over the domain, r from a mesh corner, r
    from a point outside the mesh (whose range leaves points on both sides)"""
    out = [("xyz"[a], a, 7, 0.0, 1.0, None) for a in range(dim)]
    out.append(("r-corner", 3, 7, 0.0, float(np.sqrt(dim)), (0.0, 0.0, 0.0)[:dim]))
    out.append(("r-outside", 3, 7, 0.75, 1.5, (-0.5, -0.25, -0.125)[:dim]))
    return out


def reference(d, spec, S=None, m=None):
    """profile_ref.profile_reference of the case data d under a spec; m defaults to ones (the binning does not read it)"""
    from profile_ref import profile_reference
    _, axis, nbins, lo, hi, origin = spec
    m = np.ones(d["NE"] * d["NQ"]) if m is None else m
    return profile_reference(d["dim"], d["NE"], d["N"], d["D"], d["L"], d["h1map"], d["S"] if S is None else S, m, d["gamma"], d["W"],
                             d["B"], d["G"], d["Bl"], axis, nbins, lo, hi, origin)
