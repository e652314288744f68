"""numpy restatement of the state fingerprint (include/lgh_fingerprint.h) in uint64 wrap-around arithmetic, and the inputs
the CPU and GPU tests share."""
import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
OFFSETS = (0, 1, 2 ** 40 + 3)


def fp_ref(words, offset=0):
    """(sum word, xor word) of the 64-bit words of `words` (float64 / int64 / uint64), the first at position `offset`"""
    w = np.ascontiguousarray(words).view(np.uint64).reshape(-1)
    with np.errstate(over="ignore"):
        i = np.arange(w.size, dtype=np.uint64) + np.uint64(offset) + np.uint64(1)
        z = w + i * GOLDEN
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
        return int(np.add.reduce(z, dtype=np.uint64)), int(np.bitwise_xor.reduce(z, dtype=np.uint64) if z.size else 0)


def combine(a, b):
    """the fingerprint of a concatenation from those of its parts (each taken at its offset)"""
    return (a[0] + b[0]) % 2 ** 64, a[1] ^ b[1]


def special_values():
    """-0.0, infinities, a NaN with a payload, the default NaN, denormals, among ordinary numbers"""
    bits = np.array([0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF80000DEADBEEF, 0x7FF8000000000000,
                     0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x0000000000000000, 0x3FF0000000000000, 0xBFF8000000000000,
                     0x7FF0000000000001], dtype=np.uint64)
    return bits.view(np.float64)


def data(n, seed=0):
    """n doubles: random bit patterns of ordinary size, with the special values spread in where there is room"""
    rng = np.random.default_rng(seed + 7 * n)
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
    sp = special_values()
    if n >= 2 * sp.size:
        x[rng.choice(n, sp.size, replace=False)] = sp
    return x
