"""numpy restatement of lgh_profile for the tests: the point values of tests/diag_ref.py and the position of every point by
a dense einsum, the bin index by the formula of include/laghos_hip.h, and per row and column math.fsum of the addends (the
correctly rounded sum) beside the sum of their absolute values, which the bounds of the tests are made of.  Shares no code
with the library.  m_q (rho0DetJ0w) is an input, as in diag_ref.

Also the reader of the `-prof` files the driver tests use (read_profile)."""
import math

import numpy as np

from diag_ref import _interp, point_values

COLS = ("n", "vol", "mass", "ie", "ke", "mom", "pv", "mxi", "rho_min", "rho_max")
SUM_COLS = (1, 2, 3, 4, 5, 6, 7)
AXES = {"x": 0, "y": 1, "z": 2, "r": 3}
FILE_COLUMNS = ("row", "lo", "hi") + COLS + ("rho", "e", "v", "p", "xi")
EXACT_COLUMNS = ("rho_exact", "v_exact", "p_exact")
HEAD_KEYS = ("cycle", "t", "axis", "origin_x", "origin_y", "origin_z", "lo", "hi", "nbins", "n_excluded")


def positions(dim, NE, N, D1D, h1map, S, B):
    """x_q = x_first + sum B (x - x_first): [dim, NE, NQ]"""
    hm = np.asarray(h1map).reshape(NE, *([D1D] * dim))
    out = []
    for c in range(dim):
        xc = S[c * N:(c + 1) * N][hm]
        first = xc.reshape(NE, -1)[:, 0]
        out.append(first[:, None] + _interp(xc - first.reshape(NE, *([1] * dim)), [B] * dim, dim))
    return np.stack(out)


def profile_reference(dim, NE, N, D1D, L1D, h1map, S, m, gamma, W, B, G, Bl, axis, nbins, lo, hi, origin=None):
    """dict rows [nbins + 2, 10], abs [nbins + 2, 10] (sum |addend| in the sum columns), cond (the same with every interpolated
    factor replaced by its interpolation of absolute values: >= abs), n_excluded, kappa, and the point arrays
    [NE, NQ]: xi, row (-1: excluded), s = (xi - lo) inv_w, detJ, r_small (axis r: r_q / h), mom_extra [nbins + 2]"""
    axis = AXES.get(axis, axis)
    pv = point_values(dim, NE, N, D1D, L1D, h1map, S, B, G, Bl)
    det, e, v = pv["detJ"], pv["e"], pv["v"]
    NQ = det.shape[1]
    x = positions(dim, NE, N, D1D, h1map, S, B)
    # the interpolations with absolute values throughout: what a point value is conditioned by (a v_q of 216 random dofs is far
    # smaller than sum |B| |v_d|, and its rounding error is relative to the latter)
    hm = np.asarray(h1map).reshape(NE, *([D1D] * dim))
    H1V = dim * N
    with np.errstate(all="ignore"):
        A_v = np.stack([_interp(np.abs(S[H1V + c * N:H1V + (c + 1) * N][hm]), [np.abs(B)] * dim, dim) for c in range(dim)])
        A_e = _interp(np.abs(S[2 * H1V:].reshape(NE, *([L1D] * dim))), [np.abs(Bl)] * dim, dim)
        A_x = []
        for c in range(dim):
            xc = S[c * N:(c + 1) * N][hm]
            first = xc.reshape(NE, -1)[:, 0]
            A_x.append(np.abs(first)[:, None] + _interp(np.abs(xc - first.reshape(NE, *([1] * dim))), [np.abs(B)] * dim, dim))
        A_x = np.stack(A_x)
    m = np.asarray(m).reshape(NE, NQ)
    w = np.asarray(W).reshape(1, NQ)
    gm1 = np.asarray(gamma).reshape(NE, 1) - 1.0
    o = np.zeros(3) if origin is None else np.asarray(origin, dtype=np.float64)
    inv_w = nbins / (hi - lo)
    with np.errstate(all="ignore"):
        if axis < 3:
            xi, vn, d1 = x[axis], v[axis], np.ones_like(det)
        else:
            d = x - o[:dim, None, None]
            xi = np.sqrt((d * d).sum(axis=0))
            vn = np.where(xi > 0.0, (v * d).sum(axis=0) / xi, 0.0)
            d1 = np.abs(d).sum(axis=0)
        v2 = (v * v).sum(axis=0)
        ok = np.isfinite(det) & np.isfinite(e) & np.isfinite(v).all(axis=0) & np.isfinite(xi) & (det > 0.0)
        rho = m / (w * det)
        p = gm1 * rho * np.maximum(e, 0.0)
        s = (xi - lo) * inv_w
        b = np.floor(s)
        row = np.where(b < 0, 0, np.where(b >= nbins, nbins + 1, 1 + np.clip(np.nan_to_num(b), 0, nbins - 1))).astype(np.int64)
        row = np.where(ok, row, -1)
        add = {1: w * det, 2: m + 0.0 * det, 3: m * e, 4: 0.5 * m * v2, 5: m * vn, 6: w * det * p, 7: m * xi}
        mv = m * np.sqrt(v2)
        if axis < 3:
            c_mom, c_xi = m * A_v[axis], m * A_x[axis]
        else:
            reach = A_x + np.abs(o[:dim, None, None])
            c_mom, c_xi = m * (A_v * reach).sum(axis=0) / xi, m * reach.sum(axis=0)
        cond = {1: np.abs(w * det), 2: np.abs(m + 0.0 * det), 3: m * A_e, 4: 0.5 * m * (A_v * A_v).sum(axis=0), 5: c_mom,
                6: np.abs(gm1) * m * A_e, 7: c_xi}
    R = nbins + 2
    rows, ab, cd, mom_extra = np.zeros((R, 10)), np.zeros((R, 10)), np.zeros((R, 10)), np.zeros(R)
    rows[:, 8], rows[:, 9] = np.inf, -np.inf
    flat_row = row.reshape(-1)
    order = np.argsort(flat_row, kind="stable")
    sorted_rows = flat_row[order]
    for r in np.unique(sorted_rows):
        if r < 0:
            continue
        idx = order[np.searchsorted(sorted_rows, r, "left"):np.searchsorted(sorted_rows, r, "right")]
        rows[r, 0] = len(idx)
        for k in SUM_COLS:
            t = add[k].reshape(-1)[idx]
            rows[r, k] = math.fsum(t) if np.isfinite(t).all() else np.nan
            ab[r, k] = math.fsum(np.abs(t)) if np.isfinite(t).all() else np.inf
            tc = cond[k].reshape(-1)[idx]
            cd[r, k] = math.fsum(tc) if np.isfinite(tc).all() else np.inf
        rr = rho.reshape(-1)[idx]
        rows[r, 8], rows[r, 9] = rr.min(), rr.max()
        if axis == 3:
            with np.errstate(all="ignore"):
                mom_extra[r] = d1.reshape(-1)[idx].max() * math.fsum(mv.reshape(-1)[idx] / xi.reshape(-1)[idx])
    # the smallest extent of a zone along an axis: the scale below which a radius is "at the origin"
    hm = hm.reshape(NE, -1)
    with np.errstate(all="ignore"):
        ext = np.stack([np.ptp(S[c * N:(c + 1) * N][hm], axis=1) for c in range(dim)])
    h = float(np.nanmin(ext)) if np.isfinite(ext).any() else 1.0
    return dict(rows=rows, abs=ab, cond=cd, n_excluded=int((~ok).sum()), kappa=pv["kappa"], xi=xi, row=row, s=s, detJ=det, ok=ok,
                r_over_h=(xi / h if axis == 3 else None), mom_extra=mom_extra, axis=axis, nbins=nbins, e=e, rho=rho)


def undecided(ref):
    """the number of points whose row, or whose place among the excluded, hangs on a rounding: (xi - lo) inv_w within 1e-9 of
    an integer, |detJ| < 1e-9 max |detJ|, or (axis r) r < 1e-6 h"""
    with np.errstate(all="ignore"):
        s, det = ref["s"], ref["detJ"]
        fin = np.isfinite(s) & np.isfinite(det)
        bad = fin & (np.abs(s - np.rint(s)) < 1e-9)
        bad |= fin & (np.abs(det) < 1e-9 * np.nanmax(np.abs(det)))
        if ref["r_over_h"] is not None:
            bad |= fin & (ref["r_over_h"] < 1e-6)
    return int(bad.sum())


def read_profile(path):
    """a `-prof` file: (head: dict of the values of line 1, columns: the names of line 2, rows: list of dicts, lines: raw).
    Integers (cycle, nbins, n_excluded, row, n) come back as ints, the axis as its letter, everything else as floats."""
    lines = open(path).read().splitlines(keepends=True)
    assert len(lines) >= 2 and all(l.endswith("\n") for l in lines)
    cells = lines[0].split()
    assert cells[0] == "#" and tuple(cells[1:1 + len(HEAD_KEYS)]) == HEAD_KEYS and len(cells) == 1 + 2 * len(HEAD_KEYS), lines[0]
    head = {}
    for k, c in zip(HEAD_KEYS, cells[1 + len(HEAD_KEYS):]):
        head[k] = c if k == "axis" else (int(c) if k in ("cycle", "nbins", "n_excluded") else float(c))
    columns = tuple(lines[1].split())
    assert columns in (FILE_COLUMNS, FILE_COLUMNS + EXACT_COLUMNS), lines[1]
    rows = []
    for l in lines[2:]:
        c = l.split()
        assert len(c) == len(columns), l
        rows.append({k: (int(x) if k in ("row", "n") else float(x)) for k, x in zip(columns, c)})
    assert len(rows) == head["nbins"] + 2
    return head, columns, rows, lines


def fmt(v):
    """a double as the driver prints it"""
    return "nan" if np.isnan(v) else "%.17g" % v


def format_row(r, nbins, lo, hi, d, exact=None):
    """one table row of a `-prof` file, with its newline, from the 10 doubles of a row of lgh_profile"""
    e0 = -np.inf if r == 0 else lo + (hi - lo) * float(r - 1) / float(nbins)
    e1 = np.inf if r == nbins + 1 else lo + (hi - lo) * float(r) / float(nbins)
    ratio = lambda a, b: a / b if b != 0.0 else np.nan
    with np.errstate(all="ignore"):
        cells = [str(r), fmt(e0), fmt(e1), str(int(d[0]))] + [fmt(x) for x in d[1:]]
        cells += [fmt(np.float64(ratio(d[2], d[1]))), fmt(np.float64(ratio(d[3], d[2]))), fmt(np.float64(ratio(d[5], d[2]))),
                  fmt(np.float64(ratio(d[6], d[1]))), fmt(np.float64(ratio(d[7], d[2])))]
    if exact is not None:
        cells += [fmt(x) for x in exact]
    return " ".join(cells) + "\n"
