"""numpy restatement of lgh_loads (include/laghos_hip.h) for the tests, and the cases both test files run on.  Shares no code
with the library.

The traces on a face are evaluated with the FULL-ZONE tables - on the normal axis the row of the end point xi = s of the
tables of tests/derived_ref.py, on the tangential axes the Gauss tables of the discretisation - not with the end-point
shortcut of the kernel; N is row a of adj(J) (tests/faces_ref.py adjugate) of the whole Jacobian, signed by the side;
p = (gamma - 1) rho max(e, 0).  One thing is taken from the definition and not from the tables: a dof that an EXACT zero
of the end-point row multiplies is no part of a trace, so a NaN elsewhere in the zone stays out of it.  The per-row sums
and the sums of |addend| are math.fsum.

Bound (EPS = 2^-52):  |got - want| <= 2 C kappa EPS sum |addend|,  C = (dim + 2) D1D^(dim-1) + 2 L1D^(dim-1) + 16 - the
rounded operations behind one addend: two tangents, x or v, e and rho, the products; the factor 2 for the kernel once and
numpy once; kappa = max(1, max N_abs / |N|) over the row's points, N_abs the formula of N with every term - down to the
products of table entries and node offsets x - x_first - replaced by its absolute value (the conditioning argument of
DESIGN.md 7a for J).
Extremes: |got - want| <= 2 C EPS pscale, pscale = max over the row's faces of |gamma - 1| max |rho dof| max |e dof| of the
zone - the traces of e and rho are sums of at most L1D^(dim-1) products of Bernstein values (non-negative, adding up to
one) with dofs, and p is two products on top."""
import math

import numpy as np

from derived_ref import _contract, _jacobian, lattice_tables3
from faces_ref import adjugate

EPS = 2.0 ** -52
COLS = ("n", "area", "force_x", "force_y", "force_z", "pa", "power", "flux", "xn", "p_min", "p_max")
SUM_COLS = range(1, 9)

ZONES = {"2D-1x1": (1, 1), "2D-3x2": (3, 2), "3D-1x1x1": (1, 1, 1), "3D-3x2x2": (3, 2, 2), "3D-5x5x3": (5, 5, 3)}
SMALL = ("2D-1x1", "2D-3x2", "3D-1x1x1")
CASES = [(z, o) for z in ZONES for o in [(1, 0), (2, 1), (3, 2)]] + [(z, (4, 3)) for z in SMALL]
IDS = [f"{z}-Q{o[0]}Q{o[1]}" for z, o in CASES]


def C_ops(dim, D, L):
    return (dim + 2) * D ** (dim - 1) + 2 * L ** (dim - 1) + 16


def bound(dim, D, L, kappa, abs_sum):
    return 2.0 * C_ops(dim, D, L) * kappa * EPS * abs_sum


def case_data(zones, ok, ot, seed=3):
    """The discretisation on `zones` unit-box zones, its curved initial mesh (helpers.CurvedInitialMesh) and the state
    helpers.deformed_state on it; density dofs that are not constant; made without a GPU.  Lexicographic numbering."""
    from helpers import CurvedInitialMesh, deformed_state
    from oracle.fem import Problem
    p = Problem(breaks=[np.linspace(0.0, 1.0, n + 1) for n in zones], order_v=ok, order_e=ot, problem=1)
    curved = CurvedInitialMesh(p)
    S = deformed_state(curved, seed=seed)
    _, rho0, gamma, _ = curved.initial_state()
    rng = np.random.default_rng(100 * len(zones) + 10 * ok + p.NE)
    rho = np.asarray(rho0) * rng.uniform(0.5, 2.0, p.L2V)
    w1 = np.asarray(p.qwts, dtype=np.float64)
    S0, _, _, rho0_q = curved.initial_state()
    return dict(x0=S0[:p.H1V].copy(), rho0_l2=np.asarray(rho0), rho0_q=np.asarray(rho0_q), dim=p.dim, NE=p.NE, N=p.N, D=p.D1D, L=p.L1D, Q=p.Q1D, ok=ok, ot=ot, zones=tuple(zones), h1map=np.asarray(p.h1map).reshape(-1).astype(np.int32),
                S=S, rho=rho, gamma=np.asarray(gamma, dtype=np.float64).copy(), B=np.asarray(p.B), G=np.asarray(p.G), Bl=np.asarray(p.Bl), w1=w1,
                W=np.asarray(p.W), ess=p.ess, prob=p)


def all_faces(d):
    dim, NE = d["dim"], d["NE"]
    return np.stack([np.repeat(np.arange(NE), 2 * dim), np.tile(np.arange(2 * dim), NE)], 1).astype(np.int32)


def boundary_faces(d):
    from faces_ref import brute_boundary_faces
    return brute_boundary_faces(d["dim"], d["NE"], d["D"], d["h1map"])


def wall_groups(d, faces=None):
    """[(name, faces)]: the surface, then the walls x0 x1 y0 y1 [z0 z1] - the boundary faces split by local face (on these
    structured meshes local face 2a + s on the boundary is side s of axis a of the box)"""
    bf = boundary_faces(d) if faces is None else faces
    return [("surface", bf)] + [("xyz"[f >> 1] + str(f & 1), bf[bf[:, 1] == f]) for f in range(2 * d["dim"])]


def listing(groups):
    """the (nfaces, 3) list of a sequence of groups: group r under row r"""
    return np.concatenate([np.concatenate([np.asarray(f, np.int32).reshape(-1, 2), np.full((len(f), 1), r, np.int32)], 1) for r, (_, f) in enumerate(groups)])


class FacePoints:
    """The point quantities of every face (e, f) asked for, evaluated once per face and state and shared."""

    def __init__(self, d, S=None, rho=None, gamma=None):
        self.d = d
        self.S = np.asarray(d["S"] if S is None else S, dtype=np.float64)
        self.rho = np.asarray(d["rho"] if rho is None else rho, dtype=np.float64)
        self.gamma = np.asarray(d["gamma"] if gamma is None else gamma, dtype=np.float64)
        self.E = lattice_tables3(d["ok"], d["ot"], 1)   # the tables at xi = 0 and 1: rows 0, 1
        self._made = {}

    def face(self, e, f):
        key = (int(e), int(f))
        if key not in self._made:
            self._made[key] = self._evaluate(*key)
        return self._made[key]

    def _evaluate(self, e, f):
        d = self.d
        dim, N, D, L, Q = d["dim"], d["N"], d["D"], d["L"], d["Q"]
        a, s = f >> 1, f & 1
        H1V, NL = dim * N, L ** dim
        hm = d["h1map"].reshape(d["NE"], *([D] * dim))[e:e + 1]
        Eb, Eg, El = self.E
        Bt = [Eb[s:s + 1] if ax == a else d["B"] for ax in range(dim)]       # values per axis
        Gt = [Eg[s:s + 1] if ax == a else d["G"] for ax in range(dim)]
        Lt = [El[s:s + 1] if ax == a else d["Bl"] for ax in range(dim)]
        X, V = self.S[:H1V].reshape(dim, N), self.S[H1V:2 * H1V].reshape(dim, N)

        def cube(U, row):
            """the zone's dofs with those an EXACT zero of the end-point row annihilates set to zero: a trace is a function of the
            face layer, and a dof that is not finite elsewhere in the zone (0 * NaN) is no part of it"""
            shape = [1] * (dim + 1)
            shape[dim - a] = row.size
            return np.where((row == 0).reshape(shape), 0.0, U)
        with np.errstate(all="ignore"):
            x = np.stack([_contract(cube(X[c][hm], Eb[s]), Bt, dim) for c in range(dim)], 1)
            v = np.stack([_contract(cube(V[c][hm], Eb[s]), Bt, dim) for c in range(dim)], 1)
            ev = _contract(cube(self.S[2 * H1V:].reshape(-1, *([L] * dim))[e:e + 1], El[s]), Lt, dim)
            rv = _contract(cube(self.rho.reshape(-1, *([L] * dim))[e:e + 1], El[s]), Lt, dim)

            def jac(F, absolute):
                ab = np.abs if absolute else (lambda t: t)
                return np.stack([np.stack([_contract(ab(F[i][hm]) if j == a else cube(ab(F[i][hm]), Eb[s]),
                                                     [ab(Gt[ax]) if ax == j else ab(Bt[ax]) for ax in range(dim)], dim)
                                           for j in range(dim)], -1) for i in range(dim)], 1)
            # J from the offsets from the face's first node: a derivative does not see a constant, but the entries of a
            # derivative row add up to zero only to rounding - on a flat face that noise would be all a component of N holds
            first = hm.reshape(-1)[self._first_dof(dim, D, a, s)]
            J = jac(X - X[:, first:first + 1], False)
            sgn = 1.0 if s else -1.0
            Nv = sgn * adjugate(J)[:, a, :]
            # N_abs: the same with every term absolute
            JA = jac(X - X[:, first:first + 1], True)
            JA[:, :, a] = 0.0                                                  # (row a of adj(J) has no term of column a)
            NA = self._abs_adj_row(JA, a)
            p = (self.gamma[e] - 1.0) * rv * np.maximum(ev, 0.0)
        w = d["w1"] if dim == 2 else (d["w1"][None, :] * d["w1"][:, None]).reshape(-1)    # p = q_b + Q q_c
        assert x.shape == (Q ** (dim - 1), dim) and w.shape == (Q ** (dim - 1),)
        pscale = abs(self.gamma[e] - 1.0) * np.abs(self.rho.reshape(-1, NL)[e]).max() * np.abs(self.S[2 * H1V:].reshape(-1, NL)[e]).max()
        return dict(x=x, v=v, N=Nv, NA=NA, e=ev, rho=rv, p=p, w=w, pscale=float(pscale))

    @staticmethod
    def _first_dof(dim, D, a, s):
        return s * (D - 1) * D ** a

    @staticmethod
    def _abs_adj_row(J, a):
        """row a of adj(J) with every product added instead of subtracted (J >= 0)"""
        n = J.shape[-1]
        if n == 2:
            return np.stack([J[:, 1, 1], J[:, 0, 1]], 1) if a == 0 else np.stack([J[:, 1, 0], J[:, 0, 0]], 1)
        out = np.empty((J.shape[0], 3))
        for j in range(3):
            r, q = (j + 1) % 3, (j + 2) % 3
            c, dd = (a + 1) % 3, (a + 2) % 3
            out[:, j] = J[:, r, c] * J[:, q, dd] + J[:, r, dd] * J[:, q, c]
        return out


def loads_reference(fp, faces, nrows):
    """rows (nrows, 11), abs (nrows, 11): sum |addend| per sum column, kappa (nrows), n_excluded, n_points - for the list
    `faces` (nfaces, 3) on the FacePoints fp.  A sum column with an addend that is not finite is NaN."""
    dim = fp.d["dim"]
    faces = np.asarray(faces).reshape(-1, 3)
    add = [[[] for _ in range(8)] for _ in range(nrows)]
    pmin, pmax, cnt, kap, psc = [math.inf] * nrows, [-math.inf] * nrows, [0] * nrows, [1.0] * nrows, [0.0] * nrows
    n_excl = 0
    with np.errstate(all="ignore"):
        for e, f, r in faces:
            q = fp.face(e, f)
            ok = np.isfinite(q["x"]).all(1) & np.isfinite(q["v"]).all(1) & np.isfinite(q["N"]).all(1) & np.isfinite(q["e"]) & np.isfinite(q["rho"])
            n_excl += int((~ok).sum())
            if not ok.any():
                continue
            w, p, Nv = q["w"][ok], q["p"][ok], q["N"][ok]
            nrm = np.sqrt((Nv * Nv).sum(1))
            vn, xn = (q["v"][ok] * Nv).sum(1), (q["x"][ok] * Nv).sum(1)
            wp = w * p
            cols = [w * nrm] + [wp * Nv[:, c] if c < dim else np.zeros(len(w)) for c in range(3)] + [wp * nrm, wp * vn, w * vn, w * xn]
            for k in range(8):
                add[r][k].extend(cols[k].tolist())
            cnt[r] += int(ok.sum())
            psc[r] = max(psc[r], q["pscale"])
            good = p[~np.isnan(p)]
            if good.size:
                pmin[r], pmax[r] = min(pmin[r], float(good.min())), max(pmax[r], float(good.max()))
            na = np.sqrt((q["NA"][ok] ** 2).sum(1))
            kap[r] = max(kap[r], float(np.max(na / nrm)))
    rows, ab = np.zeros((nrows, 11)), np.zeros((nrows, 11))
    for r in range(nrows):
        rows[r, 0], rows[r, 9], rows[r, 10] = cnt[r], pmin[r], pmax[r]
        for k in range(8):
            t = add[r][k]
            if all(math.isfinite(u) for u in t):
                rows[r, 1 + k], ab[r, 1 + k] = math.fsum(t), math.fsum(abs(u) for u in t)
            else:
                rows[r, 1 + k], ab[r, 1 + k] = math.nan, math.inf
    return dict(rows=rows, abs=ab, kappa=np.array(kap), pscale=np.array(psc), n_excluded=n_excl, n_points=len(faces) * fp.d["Q"] ** (dim - 1))


def volume_integrals(d, S=None):
    """sum w detJ and sum w detJ div v over the Gauss points of all zones (math.fsum), each with its sum of |terms|:
    (vol, vol_abs, dvol, dvol_abs); detJ div v = tr(adj(J) dv/dxi)"""
    dim, D = d["dim"], d["D"]
    S = np.asarray(d["S"] if S is None else S)
    hm = d["h1map"].reshape(d["NE"], *([D] * dim))
    H1V = dim * d["N"]
    X, V = S[:H1V].reshape(dim, d["N"]), S[H1V:2 * H1V].reshape(dim, d["N"])
    J, Vx = _jacobian(X, hm, d["B"], d["G"], dim), _jacobian(V, hm, d["B"], d["G"], dim)
    A = adjugate(J)
    W = np.tile(d["W"], d["NE"])
    det = (J[:, 0, :] * A[:, :, 0]).sum(-1)
    det_abs = (np.abs(J[:, 0, :]) * np.abs(A[:, :, 0])).sum(-1)
    dv_terms = np.einsum("pij,pji->pij", Vx, A).reshape(len(W), -1)
    vol = (W * det).tolist()
    dvol = (W[:, None] * dv_terms).reshape(-1).tolist()
    return math.fsum(vol), math.fsum((W * det_abs).tolist()), math.fsum(dvol), math.fsum(abs(t) for t in dvol)
