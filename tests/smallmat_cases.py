"""Inputs with prescribed spectra for the 2x2 / 3x3 routines (oracle/smallmat.hpp, lgh_smallmat.hpp), shared by
tests/test_oracle_smallmat.py (the oracle, on the CPU) and tests/test_gpu_smallmat_edges.py (the device).

A = U diag(lambda) U^T and J = U diag(sigma) V^T are formed in np.longdouble (64-bit mantissa) from rotations made
orthogonal to that precision, and rounded ONCE to fp64: the prescribed values are then the exact ones of the fp64
matrix to 0.5 ulp of its norm, and the reference owes nothing to either implementation.  Every fourth rotation is
a signed permutation matrix (the first one the identity): axis-aligned inputs, whose exact zeros off the diagonal
steer the pivot selects.  Every matrix comes at the scales 1, 0.37, 1e-150 and 1e150."""
import ctypes
import functools

import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
SCALES = (1.0, 0.37, 1e-150, 1e150)

# name -> (spectrum, relative gap between the minimum and the next value where an eigenvector comparison is well
# posed: None = repeated minimum or gap <= 1e-6, the vector is not unique (to round-off) and the residual is the test)
EIG3 = {
    "distinct": ([-1, .2, .9], 1.2),
    "double_min": ([-1, -1, .5], None),
    "double_max": ([-1, .5, .5], 1.5),
    "triple": ([.7, .7, .7], None),
    "kernel2": ([0, 0, 1], None),
    "planar_compression": ([-1, 0, 0], 1.0),
    "gap1e-15": ([-1, LD(-1) + LD(1e-15), .5], None),
    "gap1e-10": ([-1, LD(-1) + LD(1e-10), .5], None),
    "gap1e-6": ([-1, LD(-1) + LD(1e-6), .5], None),
    "near_triple": ([1, LD(1) + LD(1e-9), LD(1) + LD(2e-9)], None),
    "indefinite": ([-1, -.13, 1], 0.87),
}
EIG2 = {
    "distinct": ([-1, .3], 1.3),
    "double": ([.4, .4], None),
    "gap1e-15": ([1, LD(1) + LD(1e-15)], None),
    "gap1e-9": ([1, LD(1) + LD(1e-9)], None),
    "kernel": ([0, 1], 1.0),
    "compression": ([-1, 0], 1.0),
}
# singular values, 3D (2D: the third one dropped).  1 + k delta straddles Q/aa^2 = LGH_SM_QTINY = 3.2e-30, delta ~ 2e-15
SV = {"identity": [1, 1, 1]}
for _d in (1e-16, 1e-15, 3e-15, 1e-14, 1e-12, 1e-8, 1e-3):
    SV[f"1+k*{_d:g}"] = [1, LD(1) + LD(_d), LD(1) + 2 * LD(_d)]
SV.update({
    "double_high": [2, 2, 1],
    "double_low": [2, 1, 1],
    "cond1e4": [1, .3, 1e-4],
    "cond1e8": [1, .3, 1e-8],
    "rank_deficient": [1, .5, 0],
    "zone_h.25": [.25, .25, .25],       # diag(h) of real zone widths (cube01_hex rs2; box01_hex)
    "zone_h1_1.5": [1, 1.5, 1.5],
})
N_ZERO = 37  # zero matrices at the end: total counts are odd, no multiple of 64 or 128


def rotations(dim, n, seed):
    """n orthogonal dim x dim matrices (longdouble, orthogonal to ~1e-19): seeded QR; every fourth a signed
    permutation, the first the identity"""
    rng = np.random.default_rng(seed)
    q, r = np.linalg.qr(rng.standard_normal((n, dim, dim)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    for i in range(0, n, 4):
        P = np.zeros((dim, dim))
        P[rng.permutation(dim), np.arange(dim)] = rng.choice([-1.0, 1.0], dim)
        q[i] = P
    q[0] = np.eye(dim)
    U = q.astype(LD)
    eye3 = 3 * np.eye(dim, dtype=LD)
    for _ in range(2):  # Newton step towards the orthogonal polar factor, in extended precision
        U = np.einsum("nij,njk->nik", U, (eye3 - np.einsum("nji,njk->nik", U, U)) / 2)
    return U


class Cases:
    """M (n, dim, dim) fp64 inputs; val (n, dim) prescribed values ascending (longdouble); fam (n,) family index;
    names; norm (n,) the prescribed 2-norm (0 for the zero matrices); gap (per family) see EIG3"""

    def family(self, name):
        return np.nonzero(self.fam == self.names.index(name))[0]


def _build(dim, families, n_per, seed, symmetric):
    c = Cases()
    c.dim, c.names, c.gap = dim, list(families) + ["zero"], []
    Ms, vals, fams = [], [], []
    for f, (name, spec) in enumerate(families.items()):
        if symmetric:
            spec, gap = spec
            c.gap.append(gap)
        lam = np.array([LD(s) for s in spec[:dim]], dtype=LD)
        for k, scale in enumerate(SCALES):
            U = rotations(dim, n_per, seed + 101 * f + 7 * k)
            V = U if symmetric else rotations(dim, n_per, seed + 101 * f + 7 * k + 3)
            d = lam * LD(scale)
            Ms.append(np.einsum("nij,j,nkj->nik", U, d, V).astype(np.float64))
            vals.append(np.broadcast_to(np.sort(d), (n_per, dim)))
            fams.append(np.full(n_per, f))
    c.gap.append(None)
    Ms.append(np.zeros((N_ZERO, dim, dim)))
    vals.append(np.zeros((N_ZERO, dim), dtype=LD))
    fams.append(np.full(N_ZERO, len(families)))
    c.M = np.ascontiguousarray(np.concatenate(Ms))
    c.val = np.concatenate(vals)
    c.fam = np.concatenate(fams)
    c.norm = np.abs(c.val).max(axis=1).astype(np.float64)
    if symmetric:  # the rounding to fp64 is element-wise on a symmetric longdouble product only up to its own round-off
        c.M = 0.5 * (c.M + np.transpose(c.M, (0, 2, 1)))
    return c


@functools.lru_cache(maxsize=None)
def eig_cases(dim, n_per=500):
    return _build(dim, EIG3 if dim == 3 else EIG2, n_per, 1000 * dim, True)


@functools.lru_cache(maxsize=None)
def sv_cases(dim, n_per=500):
    return _build(dim, SV, n_per, 5000 * dim, False)


def col_major(M):
    """(n, dim, dim) matrices -> the flat column-major array both implementations take"""
    return np.ascontiguousarray(np.transpose(M, (0, 2, 1))).reshape(-1)


def _oracle_lib():
    from oracle.driver import lib
    L = lib()
    for name in ("lgo_eig2", "lgo_eig3"):
        getattr(L, name).argtypes = [ctypes.c_void_p] * 3
        getattr(L, name).restype = None
    for name in ("lgo_sv2", "lgo_sv3"):
        getattr(L, name).argtypes = [ctypes.c_void_p, ctypes.c_int]
        getattr(L, name).restype = ctypes.c_double
    return L


def oracle_eig(dim, M):
    """the oracle's CalcEigenvalues on every matrix: (lam (n, dim) ascending as it returns them, vec (n, dim) of lam[0])"""
    fn = getattr(_oracle_lib(), f"lgo_eig{dim}")
    n, d2 = len(M), dim * dim
    a = col_major(M)
    lam, vec = np.zeros((n, dim)), np.zeros((n, d2))
    pa, pl, pv = a.ctypes.data, lam.ctypes.data, vec.ctypes.data
    for i in range(n):
        fn(pa + 8 * d2 * i, pl + 8 * dim * i, pv + 8 * d2 * i)
    return lam, vec[:, :dim].copy()


def oracle_sv(dim, M):
    """the oracle's CalcSingularvalue(J, dim - 1): the smallest singular value of every matrix"""
    fn = getattr(_oracle_lib(), f"lgo_sv{dim}")
    n, d2 = len(M), dim * dim
    a = col_major(M)
    pa = a.ctypes.data
    return np.array([fn(pa + 8 * d2 * i, dim - 1) for i in range(n)])


def sv_cond_factor(val):
    """max(1, s_max / max(s_min, sqrt(eps) s_max)): the routines form J^T J, so their error in s_min grows like
    eps s_max (s_max / s_min) until s_min^2 drops below the round-off of s_max^2"""
    val = np.abs(np.asarray(val, dtype=np.float64))
    smax, smin = val.max(axis=1), val.min(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = smax / np.maximum(smin, np.sqrt(EPS) * smax)
    return np.where(smax > 0, np.maximum(1.0, f), 1.0)


def per_family(cases, err_over_norm):
    """worst entry of err_over_norm in every family: {name: value}"""
    return {name: float(np.max(err_over_norm[cases.fam == f])) for f, name in enumerate(cases.names)}


def rel(err, norm):
    """err / norm, with the zero matrices' errors kept absolute"""
    return np.asarray(err, dtype=np.float64) / np.where(norm > 0, norm, 1.0)
