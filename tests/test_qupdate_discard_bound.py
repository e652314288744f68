"""The inequality behind the dt candidate's skip (qpoint_body, lgh_qpoint.hpp), on the CPU: for a matrix with det J > 0
   3D: sigma_min(J) >= 2 det J / |J|_F^2        2D: sigma_min(J) >= det J / |J|_F
so 1 / h_min <= ih_ub = ihn / ihd and inv_dt <= S ih_ub + 2.5 visc_coeff ih_ub^2 / R.  Checked against numpy's singular
values on random matrices from well conditioned to nearly singular, with the slack the kernel's margin of 1e-9 leaves
for the `regular` ones (bound on sigma_min^2 at least 1e-4 |J|_F^2).  No GPU."""
import numpy as np
import pytest


def lower_bound(J):
    dim = J.shape[0]
    det, f2 = np.linalg.det(J), float((J * J).sum())
    return (2.0 * det / f2) if dim == 3 else det / np.sqrt(f2), f2


@pytest.mark.parametrize("dim", [2, 3])
def test_sigma_min_bound(dim):
    rng = np.random.default_rng(dim)
    worst, n_regular = 0.0, 0
    for i in range(4000):
        U, _ = np.linalg.qr(rng.normal(size=(dim, dim)))
        V, _ = np.linalg.qr(rng.normal(size=(dim, dim)))
        s = np.sort(10.0 ** rng.uniform(-6 if i % 2 else -1, 1, dim))[::-1]
        if i % 7 == 0:
            s[:] = s[0]                      # all equal: the bound's slack is largest (3D: 2/3)
        if i % 11 == 0 and dim == 3:
            s[1] = s[0]                      # sigma_1 = sigma_2: the 3D bound is tight
        J = U @ np.diag(s) @ V.T
        if np.linalg.det(J) < 0:
            J[:, 0] = -J[:, 0]
        lb, f2 = lower_bound(J)
        smin = np.linalg.svd(J, compute_uv=False)[-1]
        regular = lb * lb >= 1e-4 * f2
        if regular:
            n_regular += 1
            assert lb <= smin * (1.0 + 1e-11)                 # (rounding of this check itself: cond <= ~200)
            worst = max(worst, lb / smin)
        else:
            assert lb <= smin * (1.0 + 1e-4)                  # true in exact arithmetic; here det carries cond * eps
    assert n_regular > 1000 and worst > 0.999                 # the tight case was met


def test_inverse_dt_bound_is_monotone():
    """idt(ih) = S ih + 2.5 visc ih^2 / R grows with ih for S, visc >= 0, R > 0: the bound on 1 / h_min carries over, and
    the cross-multiplied comparison of the kernel is the same statement"""
    rng = np.random.default_rng(0)
    for _ in range(2000):
        S, visc, R = rng.uniform(0, 3), rng.uniform(0, 2), rng.uniform(0.1, 5)
        ihd, ihn = rng.uniform(1e-3, 1), rng.uniform(1e-3, 1)
        ih_ub = ihn / ihd
        ih = ih_ub * rng.uniform(0.3, 1.0)
        idt, idt_ub = S * ih + 2.5 * visc * ih * ih / R, S * ih_ub + 2.5 * visc * ih_ub * ih_ub / R
        assert idt <= idt_ub * (1 + 1e-15)
        cfl, dt_ref = 0.5, rng.uniform(1e-3, 10)
        w = ihn * (S * R * ihd + 2.5 * visc * ihn)
        if cfl * R * ihd * ihd > dt_ref * (1.0 + 1e-9) * max(w, 1e-290):
            assert idt == 0.0 or cfl / idt > dt_ref
