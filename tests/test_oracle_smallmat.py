"""The oracle's own 2x2 / 3x3 routines (oracle/smallmat.hpp: CalcEigenvalues, CalcSingularvalue - the restatement of
the mfem::kernels the reference's QUpdateBody calls) against prescribed spectra and against numpy.linalg, on the
CPU.  Every device test of lgh_smallmat.hpp and of the quadrature update leans on these routines as its reference;
this file is what says they deserve it.  Inputs: tests/smallmat_cases.py (spectra prescribed in extended precision,
axis-aligned rotations included, four scales over 300 decades)."""
import numpy as np
import pytest

import smallmat_cases as sc

# Eigenvalue, residual and |v| - 1, relative to |A|: the bar test_smallmat_device holds the device to.
# Measured for the oracle over all families and scales: 3D 1.0e-15, 1.3e-15, 5.6e-16 (1.6e-15 against eigvalsh);
# 2D 2.2e-16, 3.0e-16, 2.2e-16 (4.1e-16 against eigvalsh).
EIG_TOL = 1e-14

# Singular value: |s - s_min| <= SV_C eps s_max max(1, s_max / max(s_min, sqrt(eps) s_max))   (sc.sv_cond_factor)
# Measured worst ratio |s - s_min| / (eps s_max factor) for the oracle over all families and scales:
#   3D 2.50 (zone_h.25; identity 2.03, 1+k*1e-16 1.64, rank_deficient 1.07, cond1e8 0.67, cond1e4 0.41, the rest <= 1.0)
#   2D 1.64 (1+k*3e-15, 1+k*1e-8, 1+k*1e-3)
# i.e. 5.6e-16 s_max at worst where well conditioned, 9.0e-13 at cond 1e4, 1.0e-8 at cond 1e8, 1.6e-8 rank deficient.
# SV_C = 4 x the worst of them.
SV_WORST_MEASURED = 2.50
SV_C = 4 * SV_WORST_MEASURED

# numpy.linalg.svd is the less accurate side on clustered values: LAPACK's bidiagonal QR iteration (dbdsqr) declares
# convergence at TOL = min(100, eps^-1/8) eps = 98.7 * 2^-53 = 1.1e-14 relative, and for s = 1 + k 1e-14 it returns
# the cluster's mean for all three (measured against the prescribed values: 46 * 2^-52 = 1.0e-14; mpmath's svd of
# the same fp64 matrix confirms the prescribed ones to 5e-17).  The comparison with numpy allows that on top.
NP_SVD_TOL = 1.1e-14


@pytest.mark.parametrize("dim", [2, 3])
def test_oracle_min_eigenpair(dim):
    c = sc.eig_cases(dim)
    lam, vec = sc.oracle_eig(dim, c.M)
    e_lam = sc.rel(np.abs(lam - c.val).max(axis=1), c.norm)   # all dim eigenvalues, ascending
    res = sc.rel(np.linalg.norm(np.einsum("nij,nj->ni", c.M, vec) - lam[:, :1] * vec, axis=1), c.norm)
    e_len = np.abs(np.linalg.norm(vec, axis=1) - 1.0)
    w = np.linalg.eigvalsh(c.M)
    e_np = sc.rel(np.abs(lam - w).max(axis=1), c.norm)
    for name, worst in (("lambda", e_lam), ("residual", res), ("|v|-1", e_len), ("vs eigvalsh", e_np)):
        print(f"eig{dim} {name}:", {k: f"{v:.1e}" for k, v in sc.per_family(c, worst).items()})
    assert np.all(np.isfinite(lam)) and np.all(np.isfinite(vec))
    assert e_lam.max() <= EIG_TOL
    assert res.max() <= EIG_TOL
    assert e_len.max() <= EIG_TOL
    assert e_np.max() <= EIG_TOL
    z = c.family("zero")
    assert np.all(lam[z] == 0.0)
    assert np.all(vec[z] == np.eye(dim)[0])


@pytest.mark.parametrize("dim", [2, 3])
def test_oracle_min_singular_value(dim):
    c = sc.sv_cases(dim)
    s = sc.oracle_sv(dim, c.M)
    want = c.val[:, 0]
    unit = sc.EPS * sc.sv_cond_factor(c.val)
    ratio = sc.rel(np.abs(s - want), c.norm) / unit
    s_np = np.linalg.svd(c.M, compute_uv=False)[:, -1]
    ratio_np = np.maximum(sc.rel(np.abs(s - s_np), c.norm) - NP_SVD_TOL, 0.0) / unit
    print(f"sv{dim} ratio to eps*cond:", {k: f"{v:.2f}" for k, v in sc.per_family(c, ratio).items()})
    print(f"sv{dim} vs numpy svd     :", {k: f"{v:.2f}" for k, v in sc.per_family(c, ratio_np).items()})
    print(f"sv{dim} error / s_max    :", {k: f"{v:.1e}" for k, v in sc.per_family(c, sc.rel(np.abs(s - want), c.norm)).items()})
    assert np.all(np.isfinite(s)) and np.all(s >= 0.0)
    assert ratio.max() <= SV_C
    assert ratio_np.max() <= SV_C
    assert np.all(s[c.family("zero")] == 0.0)


def test_case_generator_is_what_it_says():
    """the prescribed spectra are the matrices' own (numpy, to its round-off), the counts are ragged against the
    wavefront, and the axis-aligned quarter has exact zeros off the diagonal"""
    for dim in (2, 3):
        c = sc.eig_cases(dim)
        assert len(c.M) % 64 != 0 and len(c.M) % 128 != 0
        assert np.array_equal(c.M, np.transpose(c.M, (0, 2, 1)))
        w = np.linalg.eigvalsh(c.M)
        assert sc.rel(np.abs(w - c.val).max(axis=1), c.norm).max() < 5e-15
        off = ~np.eye(dim, dtype=bool)
        aligned = np.all(c.M[:, off] == 0.0, axis=1)
        assert aligned.sum() >= len(c.M) // 4
        j = sc.sv_cases(dim)
        assert len(j.M) % 64 != 0 and len(j.M) % 128 != 0
        sv = np.linalg.svd(j.M, compute_uv=False)
        assert sc.rel(np.abs(sv[:, ::-1] - j.val).max(axis=1), j.norm).max() < NP_SVD_TOL
