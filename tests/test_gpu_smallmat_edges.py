"""The device's 2x2 / 3x3 routines (lgh_smallmat.hpp through lgh_test_eig / lgh_test_singular, dim 2 and 3) on the
prescribed-spectrum families of tests/smallmat_cases.py: repeated and nearly repeated eigenvalues, J near h I (the
LGH_SM_QTINY path almost every point of a real run takes), |R| >= sqrt(Q^3), the deflation branches, large condition
numbers, axis-aligned inputs, the zero matrix, four scales over 300 decades - in two layouts: grouped by family (a
wavefront takes one branch together) and shuffled (every wavefront holds lanes of every branch).  The value-select
code (normalize3, kernel_vector_3s, reduce_3s) runs one instruction stream per lane, so a matrix must give the same
bits wherever it sits.  test_oracle_smallmat.py pins the oracle's routines on the same inputs on the CPU.

Measured on an MI355X (worst over the four scales, relative to |A| resp. s_max; device / oracle):
  eigenpairs   3D lambda 1.0e-15, residual 1.2e-15, |v|-1 4.4e-16, lambda against the oracle 1.2e-15, vectors 8.0e-16
               2D lambda 2.2e-16, residual 3.0e-16, |v|-1 2.2e-16, lambda against the oracle 2.7e-16, vectors 2.3e-16
  singular 3D  identity 1.8e-16 / 4.5e-16, 1+k 1e-16 2.2e-16 / 3.6e-16, 1+k 1e-15 1.09e-15 / 2.2e-16 (ratio 4.9: the
               LGH_SM_QTINY cut returns the rms of the three values, off by delta), 1+k 3e-15 ... 1e-3 2.2e-16 / 1.8 - 2.2e-16,
               double_high 2.7e-16 / 3.6e-16, double_low 3.9e-16 / 3.8e-16, cond1e4 8.1e-13 / 9.0e-13, cond1e8 8.7e-9 / 1.0e-8,
               rank_deficient 1.60e-8 / 1.59e-8, zone_h.25 1.8e-16 / 5.6e-16, zone_h1_1.5 2.2e-16 / 3.0e-16
  singular 2D  every family 1.1e-16 ... 3.6e-16, ratio 0.74 ... 1.00
Both layouts gave the same bits in every case."""
import numpy as np
import pytest

import smallmat_cases as sc
from helpers import make_gpu

pytestmark = pytest.mark.gpu

EIG_TOL = 1e-14   # relative to |A|: eigenvalue, residual, |v| - 1 (the bar of test_smallmat_device), also against the oracle
SV_FLOOR = 1e-14  # singular value: max(SV_FLOOR, 4 e_oracle) s_max per family (e_oracle: the oracle's worst error / s_max
SV_MARGIN = 4.0   # on the same inputs; 4: the device contracts FMAs, takes the 1-ulp root and refines a hardware reciprocal)


@pytest.fixture(scope="module")
def gpu():
    from oracle.fem import Problem
    g = make_gpu(Problem(mesh="cube01_hex", rs=0, order_v=1, order_e=0, problem=1))
    yield g
    g.close()


def device_eig(g, dim, M):
    import torch
    n = len(M)
    lam, vec = g.ctx.zeros(n), g.ctx.zeros(dim * n)
    Ad = g.ctx.to_dev(sc.col_major(M))
    torch.cuda.synchronize()
    g.ctx.test_eig(dim, Ad, lam, vec)
    g.ctx.sync()
    return lam.cpu().numpy(), vec.cpu().numpy().reshape(n, dim)


def device_sv(g, dim, M):
    import torch
    sv = g.ctx.zeros(len(M))
    Jd = g.ctx.to_dev(sc.col_major(M))
    torch.cuda.synchronize()
    g.ctx.test_singular(dim, Jd, sv)
    g.ctx.sync()
    return sv.cpu().numpy()


def shuffled(n):
    return np.random.default_rng(20240).permutation(n)


@pytest.mark.parametrize("dim", [2, 3])
def test_device_min_eigenpair_families(gpu, dim):
    c = sc.eig_cases(dim)
    lam, vec = device_eig(gpu, dim, c.M)
    perm = shuffled(len(c.M))
    lam_s, vec_s = device_eig(gpu, dim, c.M[perm])
    lam_o, vec_o = sc.oracle_eig(dim, c.M)

    e_lam = sc.rel(np.abs(lam - c.val[:, 0]), c.norm)
    res = sc.rel(np.linalg.norm(np.einsum("nij,nj->ni", c.M, vec) - lam[:, None] * vec, axis=1), c.norm)
    e_len = np.abs(np.linalg.norm(vec, axis=1) - 1.0)
    e_or = sc.rel(np.abs(lam - lam_o[:, 0]), c.norm)
    for name, worst in (("lambda", e_lam), ("residual", res), ("|v|-1", e_len), ("vs oracle", e_or)):
        print(f"eig{dim} {name}:", {k: f"{v:.1e}" for k, v in sc.per_family(c, worst).items()})
    assert np.all(np.isfinite(lam)) and np.all(np.isfinite(vec))
    assert e_lam.max() <= EIG_TOL
    assert res.max() <= EIG_TOL
    assert e_len.max() <= EIG_TOL
    assert e_or.max() <= EIG_TOL

    # the eigenvector against the oracle's where it is unique: both are unit vectors with residual <= EIG_TOL |A|, so
    # each lies within EIG_TOL |A| / gap of the true one (Davis-Kahan, sin theta <= |r| / gap) and within EIG_TOL of unit length
    for f, name in enumerate(c.names):
        if c.gap[f] is None:
            continue
        i = c.fam == f
        sign = np.sign(np.sum(vec[i] * vec_o[i], axis=1))[:, None]
        d = np.linalg.norm(vec[i] - sign * vec_o[i], axis=1).max()
        print(f"eig{dim} vector vs oracle, {name}: {d:.1e}")
        assert d <= 2 * EIG_TOL / c.gap[f] + 2 * EIG_TOL, name

    # the zero matrix: lambda = 0 exactly; 3D the `triple` branch (1, 0, 0) the tiny_grad shortcut of the point body
    # reproduces; 2D eigensystem2s with d12 = 0, then d0 <= d3 picks (c, -s) = (1, -0)
    z = c.family("zero")
    assert np.all(lam[z] == 0.0)
    assert np.all(vec[z] == np.eye(dim)[0])

    # same matrix, same bits, wherever it sits in the launch
    assert np.array_equal(lam_s, lam[perm])
    assert np.array_equal(vec_s, vec[perm])


@pytest.mark.parametrize("dim", [2, 3])
def test_device_min_singular_value_families(gpu, dim):
    c = sc.sv_cases(dim)
    s = device_sv(gpu, dim, c.M)
    perm = shuffled(len(c.M))
    s_s = device_sv(gpu, dim, c.M[perm])
    s_o = sc.oracle_sv(dim, c.M)
    want = c.val[:, 0]
    e_dev = sc.per_family(c, sc.rel(np.abs(s - want), c.norm))
    e_orc = sc.per_family(c, sc.rel(np.abs(s_o - want), c.norm))
    assert np.all(np.isfinite(s)) and np.all(s >= 0.0)
    bad = []
    for name in c.names:
        bar = max(SV_FLOOR, SV_MARGIN * e_orc[name])
        ratio = e_dev[name] / e_orc[name] if e_orc[name] > 0 else float("nan")
        print(f"sv{dim} {name:16s} device {e_dev[name]:.2e}  oracle {e_orc[name]:.2e}  ratio {ratio:6.2f}  bar {bar:.1e}")
        if not e_dev[name] <= bar:
            bad.append(name)
    assert not bad, bad
    assert np.all(s[c.family("zero")] == 0.0)
    assert np.array_equal(s_s, s[perm])
