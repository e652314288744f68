"""numpy restatement of lgh_records_update (include/laghos_hip.h): the running records of the driver's `-peaks`, one IEEE double
operation at a time - numpy contracts nothing - so that every column but speed_max can be held to the bit.

A block is an (8, n) array, row c = column c of the C ABI: p_max, t_p_max, impulse, p_last, rho_max, speed_max, e_max,
t_arrival."""
import numpy as np

COLS = ("p_max", "t_p_max", "impulse", "p_last", "rho_max", "speed_max", "e_max", "t_arrival")
SPEED = COLS.index("speed_max")
EXACT = [c for c in range(len(COLS)) if c != SPEED]
# the names a dump gives the columns it writes, in the order it writes them (p_last is not written)
DUMP_ARRAYS = (("peak_pressure", 0), ("peak_pressure_time", 1), ("pressure_impulse", 2), ("peak_density", 4), ("peak_speed", 5), ("peak_energy", 6))
ARRIVAL_ARRAY = ("arrival_time", 7)


def speed(v):
    """|v| of v (dim, n): the squares summed in ascending order, then the root"""
    s = v[0] * v[0]
    for c in range(1, v.shape[0]):
        s = s + v[c] * v[c]
    return np.sqrt(s)


def update(rec, p, rho, e, v, t, dtr, threshold=None, first=False):
    """the block after one update (rec is not changed; None is allowed with first)"""
    thr = np.nan if threshold is None else float(threshold)
    n = p.size
    sp = speed(v if v.ndim == 2 else v.reshape(v.size // max(n, 1), n))
    with np.errstate(invalid="ignore"):
        if first:
            assert dtr == 0.0
            return np.stack([p, np.full(n, t), np.zeros(n), p, rho, sp, e, np.where(p >= thr, t, -1.0)])
        out = rec.copy()
        up = p > rec[0]                      # strict: the first attainment keeps its time; False for a NaN sample
        out[0] = np.where(up, p, rec[0])
        out[1] = np.where(up, t, rec[1])
        h = 0.5 * dtr                        # formed once, as on the host
        out[2] = rec[2] + h * (rec[3] + p)   # add, multiply, add
        out[3] = p
        out[4] = np.where(rho > rec[4], rho, rec[4])
        out[5] = np.where(sp > rec[5], sp, rec[5])
        out[6] = np.where(e > rec[6], e, rec[6])
        out[7] = np.where((rec[7] < 0.0) & (p >= thr), t, rec[7])
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_block(got, want, dim, what=""):
    """got against want ((8, n) each): every column but speed_max bit for bit; speed_max within 4 eps relative - at most dim
    squarings and dim - 1 additions at half an ulp each, halved by the root, plus the root's own ulp, stay under 2.5 ulp, and a
    contracted sum of squares is allowed there.  A NaN speed (a NaN velocity sample at the start) must be NaN in both."""
    assert got.shape == want.shape, what
    for c in EXACT:
        assert np.array_equal(bits(got[c]), bits(want[c])), (what, COLS[c], int(np.flatnonzero(bits(got[c]) != bits(want[c]))[0]))
    g, w = got[SPEED], want[SPEED]
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan), (what, "speed_max NaN")
    err = np.abs(g[~nan] - w[~nan])
    tol = 4 * np.finfo(np.float64).eps * np.abs(w[~nan])
    assert np.all(err <= tol), (what, "speed_max", float((err / np.maximum(np.abs(w[~nan]), 1e-300)).max()))
