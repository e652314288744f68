"""numpy restatement of lgh_map for the tests: the point values of tests/diag_ref.py, the positions of tests/profile_ref.py,
the cell index by the formula of include/laghos_hip.h, and per row and column math.fsum of the addends (the correctly
rounded sum) beside the sum of their absolute values and beside the `cond` form of profile_ref (every interpolated factor
replaced by its interpolation of absolute values), which the bounds of the tests are made of.  Shares no code with the
library.  m_q (rho0DetJ0w) is an input, as in diag_ref.

point_data does what hangs on the state alone, bin_points what hangs on the grid: a test that looks at one state under several
grids evaluates the points once."""
import math

import numpy as np

from diag_ref import _interp, point_values
from profile_ref import positions

COLS = ("n", "vol", "mass", "ie", "ke", "mom_x", "mom_y", "mom_z", "pv", "rho_min", "rho_max")
SUM_COLS = (1, 2, 3, 4, 5, 6, 7, 8)
NCOLS = len(COLS)


def point_data(dim, NE, N, D1D, L1D, h1map, S, m, gamma, W, B, G, Bl):
    """dict x [dim, NE, NQ], ok, detJ, rho [NE, NQ], add and cond {column: [NE, NQ]}, kappa, n_excluded"""
    pv = point_values(dim, NE, N, D1D, L1D, h1map, S, B, G, Bl)
    det, e, v = pv["detJ"], pv["e"], pv["v"]
    NQ = det.shape[1]
    x = positions(dim, NE, N, D1D, h1map, S, B)
    hm = np.asarray(h1map).reshape(NE, *([D1D] * dim))
    H1V = dim * N
    m = np.asarray(m).reshape(NE, NQ)
    w = np.asarray(W).reshape(1, NQ)
    gm1 = np.asarray(gamma).reshape(NE, 1) - 1.0
    zero = np.zeros_like(det)
    with np.errstate(all="ignore"):
        A_v = np.stack([_interp(np.abs(S[H1V + c * N:H1V + (c + 1) * N][hm]), [np.abs(B)] * dim, dim) for c in range(dim)])
        A_e = _interp(np.abs(S[2 * H1V:].reshape(NE, *([L1D] * dim))), [np.abs(Bl)] * dim, dim)
        v2 = (v * v).sum(axis=0)
        ok = np.isfinite(det) & np.isfinite(e) & np.isfinite(v).all(axis=0) & np.isfinite(x).all(axis=0) & (det > 0.0)
        rho = m / (w * det)
        p = gm1 * rho * np.maximum(e, 0.0)
        add = {1: w * det, 2: m + 0.0 * det, 3: m * e, 4: 0.5 * m * v2, 8: w * det * p}
        cond = {1: np.abs(w * det), 2: np.abs(m + 0.0 * det), 3: m * A_e, 4: 0.5 * m * (A_v * A_v).sum(axis=0), 8: np.abs(gm1) * m * A_e}
        for c in range(3):
            add[5 + c] = m * v[c] if c < dim else zero
            cond[5 + c] = m * A_v[c] if c < dim else zero
    return dict(dim=dim, x=x, ok=ok, detJ=det, rho=rho, add=add, cond=cond, kappa=pv["kappa"], n_excluded=int((~ok).sum()), e=e)


def _row_sums(values, order, starts, ends, poison):
    """per run [starts[i], ends[i]) of the points in `order`: fsum of the values; `poison` where one of them is not finite"""
    t = values.reshape(-1)[order]
    fin = np.isfinite(t)
    lst = np.where(fin, t, 0.0).tolist()
    out = np.array([math.fsum(lst[a:b]) for a, b in zip(starts, ends)])
    bad = np.add.reduceat((~fin).astype(np.int64), starts) > 0 if len(starts) else np.zeros(0, dtype=bool)
    out[bad] = poison
    return out


def bin_points(pd, cells, lo, hi):
    """dict rows, abs, cond [ncells + 1, 11], n_excluded, kappa, and per point s [dim, NE, NQ] = (x - lo) inv_w, row (-1:
    excluded), detJ, ok"""
    dim = pd["dim"]
    n = [int(k) for k in cells] + [1] * (3 - len(cells))
    assert all(k == 1 for k in n[dim:])
    x, ok = pd["x"], pd["ok"]
    with np.errstate(all="ignore"):
        s = np.stack([(x[c] - lo[c]) * (n[c] / (hi[c] - lo[c])) for c in range(dim)])
        b = np.floor(s)
        inside = np.ones_like(ok)
        cell = np.zeros(ok.shape, dtype=np.int64)
        stride = 1
        for c in range(dim):
            in_c = (b[c] >= 0) & (b[c] < n[c])
            inside &= in_c
            cell += stride * np.where(in_c, np.nan_to_num(b[c]), 0).astype(np.int64)
            stride *= n[c]
    row = np.where(ok, np.where(inside, 1 + cell, 0), -1)
    R = n[0] * n[1] * n[2] + 1
    rows, ab, cd = np.zeros((R, NCOLS)), np.zeros((R, NCOLS)), np.zeros((R, NCOLS))
    rows[:, 9], rows[:, 10] = np.inf, -np.inf
    flat = row.reshape(-1)
    order = np.argsort(flat, kind="stable")
    order = order[np.searchsorted(flat[order], 0, "left"):]
    sorted_rows = flat[order]
    uniq, starts = np.unique(sorted_rows, return_index=True)
    ends = np.append(starts[1:], len(sorted_rows))
    if len(uniq):
        rows[uniq, 0] = ends - starts
        for k in SUM_COLS:
            rows[uniq, k] = _row_sums(pd["add"][k], order, starts, ends, np.nan)
            ab[uniq, k] = _row_sums(np.abs(pd["add"][k]), order, starts, ends, np.inf)
            cd[uniq, k] = _row_sums(pd["cond"][k], order, starts, ends, np.inf)
        rr = pd["rho"].reshape(-1)[order]
        rows[uniq, 9], rows[uniq, 10] = np.minimum.reduceat(rr, starts), np.maximum.reduceat(rr, starts)
    return dict(rows=rows, abs=ab, cond=cd, n_excluded=pd["n_excluded"], kappa=pd["kappa"], s=s, row=row, detJ=pd["detJ"], ok=ok, n=n)


def map_reference(dim, NE, N, D1D, L1D, h1map, S, m, gamma, W, B, G, Bl, cells, lo, hi):
    return bin_points(point_data(dim, NE, N, D1D, L1D, h1map, S, m, gamma, W, B, G, Bl), cells, lo, hi)


def undecided(ref):
    """the number of points whose row, or whose place among the excluded, hangs on a rounding: on some axis (x - lo) inv_w
    within 1e-9 of an integer, or |detJ| < 1e-9 max |detJ| (the rule of profile_ref.undecided, per axis)"""
    with np.errstate(all="ignore"):
        s, det = ref["s"], ref["detJ"]
        fin = np.isfinite(s).all(axis=0) & np.isfinite(det)
        bad = fin & (np.abs(s - np.rint(s)) < 1e-9).any(axis=0)
        bad |= fin & (np.abs(det) < 1e-9 * np.nanmax(np.abs(det)))
    return int(bad.sum())
