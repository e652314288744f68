"""The exact integer accumulators of the velocity CG (laghos_amd/csrc/lgh_vcg.hpp: exact_scale, exact_add, wave_sum_i64,
exact_value, exact_den, exact_fold, exact_fold_lanes) on their own, through lgh_test_exact_sum, against plain Python
integers and fractions (tests/exact_ref.py).  Every (d, A d) and (r, z) of the lockstep solve on the headline path is a
sum of this kind; the header promises the same bits for every schedule, a loss below 2^(E - 128) per addend, and NaN -
never a wrong number - when an addend does not fit the window."""
import math
from fractions import Fraction

import numpy as np
import pytest

import exact_ref as ref
from helpers import make_gpu

pytestmark = pytest.mark.gpu

SCALES = [-900, 12, 900]


@pytest.fixture(scope="module")
def gpu():
    from oracle.fem import Problem
    g = make_gpu(Problem(mesh="cube01_hex", rs=0, order_v=1, order_e=0, problem=1))
    yield g
    g.close()


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


# ---------------------------------------------------------------------------------------------------------------- split
def check_split(g, vals, E):
    vals = np.asarray(vals, dtype=np.float64)
    limbs, ok = g.ctx.test_exact_split(vals, E=E)
    worst = 0
    for v, l, o in zip(vals.tolist(), limbs.tolist(), ok.tolist()):
        acc = ref.accepted(v, E)
        assert o == acc, (v, E, "accepted", o)
        if not acc:
            assert l == [0, 0, 0, 0], (v, E, "a refused addend leaves the accumulators alone", l)
            continue
        off = abs(ref.limbs_units(l) - ref.units(v, E))
        if off > worst:
            worst = off
            print(f"exact_add({v!r}, E={E}): limbs {l} are {off} units (2^{math.log2(off):.1f}) off")
        assert all(abs(x) < 2 ** 32 for x in l), (v, E, "2^31 addends must fit 64 bits", l)
    assert worst == 0


@pytest.mark.parametrize("E", SCALES)
def test_split_powers_and_window_edges(gpu, E):
    top = math.ldexp(1.0, E - 1)
    below = math.nextafter(top, 0.0)
    vals = [s * math.ldexp(1.0, k) for k in range(E - 136, E - 1) for s in (1.0, -1.0)]
    vals += [below, -below, top, -top, math.nextafter(top, math.inf), -math.nextafter(top, math.inf), 0.0, -0.0]
    vals += [math.nan, math.inf, -math.inf, 5e-324, -5e-324, 3e-310, -3e-310, 2.2250738585072014e-308, -2.2250738585072014e-308]
    check_split(gpu, vals, E)
    # (what the cases are: the largest addend is accepted, 2^(E-1) and beyond, NaN and inf are not)
    assert ref.accepted(below, E) and not ref.accepted(top, E) and not ref.accepted(-top, E)


@pytest.mark.parametrize("E", SCALES)
def test_split_negative_addends(gpu, E):
    """Negative addends are where a split by floor() goes wrong: x - floor(x) of a negative x with bits below 2^-53 of
    a top-limb unit does not fit a double (for |x| < 2^-53 it rounds to 1.0 and the next limb's conversion is out of range)."""
    u = E - 32  # a top-limb unit is 2^u
    tiny = [-2.0 ** -60, -1e-30, -2.0 ** -53, -2.0 ** -54, -(2.0 ** -53) * (1 + 2.0 ** -52), -(2.0 ** -54) * (2 - 2.0 ** -52)]
    full = [-3e-9, -0.3, -(1 + 2.0 ** -52) * 2.0 ** -20, -1234567.0 - 0.3, -(2.0 ** 31 - 1) - 1e-7, -1.0 - 2.0 ** -52, -1.0 + 2.0 ** -53]
    vals = [math.ldexp(x, u) for x in tiny + full]
    vals += [-v for v in vals]
    check_split(gpu, vals, E)


@pytest.mark.parametrize("E", SCALES)
def test_split_bits_below_the_last_limb(gpu, E):
    vals = []
    for k in (0, 1, 20, 31, 40, 51, 52):  # the lowest bit of the addend lies 52 - k binades below the last limb's unit
        for m in (1 + 2.0 ** -52, 2 - 2.0 ** -52, 1.3):
            vals += [math.ldexp(m, E - 128 + k), -math.ldexp(m, E - 128 + k)]
    vals += [math.ldexp(0.3, E - 100), math.ldexp(-0.3, E - 100), math.ldexp(0.7, E - 128), math.ldexp(-0.7, E - 128)]
    check_split(gpu, vals, E)


@pytest.mark.parametrize("E", SCALES)
def test_split_random(gpu, E):
    rng = np.random.default_rng(1000 + E)
    n = 10000
    ex = rng.integers(E - 129 - 40, E - 1, size=n)  # |v| in [2^ex, 2^(ex+1)): the window and 40 binades below it
    vals = np.ldexp(rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n), ex)
    check_split(gpu, vals, E)


# ---------------------------------------------------------------------------------------------------------------- value
def value_cases():
    rng = np.random.default_rng(77)
    M = 2 ** 32
    rows = [[0, 0, 0, 0], [1, -M, 0, 0], [-1, M - 1, M - 1, M], [0, 0, 1, -M],
            [-1, M - 1, M - 1, M - 1], [-1, 0, 0, 0], [0, 0, 0, -1], [0, 0, 0, 1], [0, -1, 0, 0],
            [2 ** 53 + 1, 0, 0, 0], [2 ** 60 + 12345, 1, 2, 3], [-(2 ** 55 + 3), 7, 0, 9], [2 ** 62 - 1, M - 1, M - 1, M - 1],
            [-(2 ** 62), 2 ** 62, -(2 ** 62), 2 ** 62], [2 ** 31 - 1, M - 1, M - 1, M - 1], [-(2 ** 31), 0, 0, 0]]
    for _ in range(200):  # normalised
        rows.append([int(rng.integers(-2 ** 31, 2 ** 31))] + [int(x) for x in rng.integers(0, M, 3)])
    for _ in range(200):  # negative limbs
        rows.append([int(x) for x in rng.integers(-M, M, 4)])
    for _ in range(300):  # un-normalised: up to 2^62 in magnitude
        sh = rng.integers(0, 63, 4)
        rows.append([int(x) >> int(63 - s) for x, s in zip(rng.integers(-2 ** 63, 2 ** 63, 4), sh)])
    for _ in range(100):  # a top limb beyond 2^53
        rows.append([int(rng.integers(2 ** 53, 2 ** 62)) * int(rng.choice([-1, 1]))] + [int(x) for x in rng.integers(0, M, 3)])
    for _ in range(100):  # totals near zero of either sign: a small top limb that the lower ones almost cancel
        rows.append([int(rng.integers(-3, 4)), int(rng.integers(-2 * M, 2 * M)), int(rng.integers(-2 ** 62, 2 ** 62)), int(rng.integers(-2 ** 62, 2 ** 62))])
    return rows


@pytest.mark.parametrize("E", SCALES)
def test_value(gpu, E):
    """exact_value against the integer the words stand for.  Tolerance from its code: after the carries the lower limbs
    and the low 26 bits m of the top limb are >= 0, and the value is the chain ((l3 + l2) + l1 + m) + h, every term
    converted and scaled exactly.
    Total >= 0: then h >= 0 too; four additions of non-negative terms, each rounding by at most half an ulp of a running
    sum that does not exceed the result: error <= 2 ulp.
    Total < 0: h < 0.  The positive part (l3, l2, l1, m) is below 2^(E-6), where an ulp is at most 2^(E-59): three
    roundings of at most 2^(E-60) each, then one rounding of the result: error <= 3 * 2^(E-60) + ulp(result) / 2.  (Relative
    to a negative total close to zero that is large: the sums the solve folds, (d, A d) and (r, z), are positive.)"""
    rows = value_cases()
    got = gpu.ctx.test_exact_value(np.array(rows, dtype=np.int64), E)
    kinds = set()
    for l, v in zip(rows, got.tolist()):
        exact = ref.value(ref.limbs_units(l), E)
        err, tol = abs(Fraction(v) - exact), ref.value_tolerance(exact, v, E)
        assert err <= tol, (l, E, v, float(exact), float(err / tol))
        if exact == 0:
            assert v == 0.0, (l, v)
        kinds.add((exact > 0) - (exact < 0))
    assert kinds == {-1, 0, 1}


# ---------------------------------------------------------------------------------------------------------------- scale
def test_scale(gpu):
    """exact_scale = frexp exponent + 12 for every finite rz != 0 (sign ignored), subnormal ones included, and 12 for
    rz = 0.  For inf and NaN, where the C library leaves frexp's exponent open, the device instruction returns exponent 0:
    E = 12 as well (pinned here, written down at exact_scale)."""
    rz = []
    for k in (-1074, -1073, -1060, -1023, -1022, -1021, -600, -13, -12, -1, 0, 1, 11, 52, 53, 600, 1022, 1023):
        p = math.ldexp(1.0, k)
        rz += [p, math.nextafter(p, 0.0), math.nextafter(p, math.inf)]
    rz = [x for x in rz if x != 0.0 and math.isfinite(x)]
    rz += [-x for x in rz] + [1.7976931348623157e308, 5e-324, 0.3, 7.5e-7, 123456.789]
    E = gpu.ctx.test_exact_scale(np.array(rz))
    for x, e in zip(rz, E.tolist()):
        assert e == ref.exact_scale(x), (x, e)
    assert gpu.ctx.test_exact_scale(np.array([0.0, -0.0, math.inf, -math.inf, math.nan])).tolist() == [12] * 5


@pytest.mark.parametrize("scale", [0.0, -3.0, math.inf, -math.inf, math.nan], ids=["zero", "negative", "inf", "-inf", "nan"])
def test_fold_under_a_degenerate_scale(gpu, scale):
    """A set added and folded under exact_scale(rz) of an rz no solve should see is still either the sum or NaN, never a
    finite number that is not the sum: the scale is a valid window (E = 12 for 0, inf and NaN; that of |rz| for rz < 0)."""
    E = int(gpu.ctx.test_exact_scale(np.array([scale]))[0])
    assert E == (ref.exact_scale(scale) if math.isfinite(scale) else 12)
    rng = np.random.default_rng(5)
    v = np.ldexp(rng.uniform(-1.0, 1.0, (3, 1000)), rng.integers(E - 70, E - 1, (3, 1000)))
    words, folds = gpu.ctx.test_exact_grid(v, 3, scale=scale)
    assert words[ref.FLAG_WORD] == 0
    for k in range(3):
        u = sum(ref.units(x, E) for x in v[k].tolist())
        assert ref.set_units(words.tolist(), k) == u
        for f in range(3):
            exact = ref.value(u, E)
            assert abs(Fraction(float(folds[f, k])) - exact) <= ref.value_tolerance(exact, float(folds[f, k]), E)
    v[1, 500] = math.ldexp(1.0, E - 1)  # does not fit
    words, folds = gpu.ctx.test_exact_grid(v, 3, scale=scale)
    assert words[ref.FLAG_WORD] != 0 and np.all(np.isnan(folds))


# ----------------------------------------------------------------------------------------------------------------- grid
GRID_E = 12


@pytest.fixture(scope="module")
def multiset():
    """2^16 signed addends per component over 60 binades below the top of the window, and their exact sums"""
    rng = np.random.default_rng(2024)
    n = 1 << 16
    v = np.ldexp(rng.uniform(1.0, 2.0, (3, n)) * rng.choice([-1.0, 1.0], (3, n)), rng.integers(GRID_E - 62, GRID_E - 2, (3, n)))
    u = [sum(ref.units(x, GRID_E) for x in v[k].tolist()) for k in range(3)]
    return v, u


def check_folds(folds, u, E):
    for k in range(3):
        exact = ref.value(u[k], E)
        assert bits(folds[0, k]) == bits(folds[1, k]) == bits(folds[2, k]), (k, folds[:, k])
        got = float(folds[0, k])
        assert abs(Fraction(got) - exact) <= ref.value_tolerance(exact, got, E), (k, got, float(exact))


def test_grid_order_and_partition_independence(gpu, multiset):
    v, u = multiset
    rng = np.random.default_rng(9)
    perms = [np.arange(v.shape[1])] + [rng.permutation(v.shape[1]) for _ in range(2)]
    seen = set()
    for G in (1, 3, 4, 7, 64):
        for p in perms:
            words, folds = gpu.ctx.test_exact_grid(np.ascontiguousarray(v[:, p]), G, E=GRID_E)
            w = words.tolist()
            assert w[ref.FLAG_WORD] == 0
            got = [ref.set_units(w, k) for k in range(3)]
            assert got == u, (G, [a - b for a, b in zip(got, u)])
            # which shards hold something: workgroup b adds into shard b % 4
            used = [sh for sh in range(ref.SHARDS) if any(w[sh * 12: sh * 12 + 12])]
            assert used == list(range(min(G, ref.SHARDS))), (G, used)
            check_folds(folds, u, GRID_E)
            seen.add(tuple(bits(folds).reshape(-1).tolist()))
    assert len(seen) == 1  # the same bits from every schedule


@pytest.mark.parametrize("E", SCALES)
def test_grid_capacity(gpu, E):
    """2^20 times the largest addend of the window, its negative, and both alternating: summed exactly."""
    n = 1 << 20
    big = math.nextafter(math.ldexp(1.0, E - 1), 0.0)
    v = np.empty((3, n))
    v[0], v[1] = big, -big
    v[2] = np.where(np.arange(n) % 3 == 0, -big, big)
    words, folds = gpu.ctx.test_exact_grid(v, 64, E=E)
    w = words.tolist()
    ub = ref.units(big, E)
    u = [n * ub, -n * ub, (n - 2 * ((n + 2) // 3)) * ub]
    assert w[ref.FLAG_WORD] == 0 and [ref.set_units(w, k) for k in range(3)] == u
    check_folds(folds, u, E)


@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf, math.ldexp(1.0, GRID_E - 1), -math.ldexp(1.0, GRID_E - 1)],
                         ids=["nan", "inf", "-inf", "top", "-top"])
def test_grid_flag(gpu, multiset, bad):
    """One refused addend anywhere, in any workgroup and any component, turns all three folds of all three components
    into NaN (one flag word per set); the accepted addends are still added; the next call, on a cleared set, is clean."""
    v, u = multiset
    n = v.shape[1]
    G = 7
    for k, i in ((0, 0), (1, 256 * 3 + 70), (2, n - 1), (1, 256 * G * 5 + 256 * 6 + 255)):
        w = v.copy()
        w[k, i] = bad
        words, folds = gpu.ctx.test_exact_grid(w, G, E=GRID_E)
        assert words[ref.FLAG_WORD] != 0 and np.all(np.isnan(folds)), (k, i, folds)
        got = [ref.set_units(words.tolist(), c) for c in range(3)]
        assert got == [u[c] - (ref.units(float(v[k, i]), GRID_E) if c == k else 0) for c in range(3)]
    words, folds = gpu.ctx.test_exact_grid(v, G, E=GRID_E)
    assert words[ref.FLAG_WORD] == 0
    check_folds(folds, u, GRID_E)


# ----------------------------------------------------------------------------------------------------------------- wave
def test_wave_sum(gpu):
    """wave_sum_i64: the sum of the 64 lanes' words modulo 2^64, in every lane."""
    rng = np.random.default_rng(31)
    lo, hi = -2 ** 63, 2 ** 63 - 1
    cases = [[0xFFFFFFFF] * 64, [0xFFFFFFFF if i % 2 else 1 for i in range(64)], [-1] * 64, [(-1) ** i * (i + 1) * 0x80000001 for i in range(64)],
             [lo] * 64, [hi] * 64, [lo if i % 2 else hi for i in range(64)], [hi] * 63 + [lo], [lo] + [0] * 63, [0] * 63 + [hi],
             [1 << i for i in range(63)] + [lo], [i for i in range(64)], [0] * 64]
    for l in range(64):  # one word alone, in every lane
        cases.append([(0x123456789ABCDEF if i == l else 0) for i in range(64)])
    cases += [[int(x) for x in rng.integers(lo, hi, 64, endpoint=True)] for _ in range(20)]
    cases += [[int(x) for x in rng.integers(-2 ** 33, 2 ** 33, 64)] for _ in range(20)]
    out = gpu.ctx.test_wave_sum(np.array(cases, dtype=np.int64))
    for c, o in zip(cases, out.tolist()):
        s = (sum(c) + 2 ** 63) % 2 ** 64 - 2 ** 63
        assert o == [s] * 64, (c[:4], s, o[:4])
