"""lgh_vec_fingerprint (laghos_amd/csrc/lgh_fingerprint.hip) through Context.fingerprint against the numpy restatement of
the function (tests/fingerprint_ref.py): every size at which the kernel changes shape, slices that are only 8-byte aligned,
offsets, special values, the concatenation rule, and that the call reads its input and nothing else.  Equality is exact:
the fingerprint is two integers.  The kernel does not look at the mesh: any small context will do."""
import ctypes

import numpy as np
import pytest

from fingerprint_ref import OFFSETS, combine, data, fp_ref, special_values

pytestmark = pytest.mark.gpu

SMALL = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 65537)
MAX_N = 2 ** 22 + 5


@pytest.fixture(scope="module")
def gpu():
    from helpers import make_gpu
    from oracle.fem import Problem
    prob = Problem(mesh="cube01_hex", rs=0, order_v=2, order_e=1, problem=1)
    g = make_gpu(prob)
    g.test_prob = prob
    yield g
    g.close()


@pytest.fixture(scope="module")
def vec(gpu):
    """(host array, the same on the device, sizes beyond one pass of the grid): the host array is made once and never changed"""
    ctx = gpu.ctx
    host = data(MAX_N + 3, seed=11)
    dev = ctx.to_dev(host)
    blocks, threads, head, full = ctx.fingerprint_shape(dev)
    assert threads == 256 and head == 0 and blocks * threads * 2 == full
    # one pass of the largest grid takes `full` words: full + 5 sends some threads round a second time (the single-load loop),
    # 4 * full + 5 sends every thread through the loop with four loads in flight and some through the one after it
    big = sorted({min(full + 5, MAX_N), min(4 * full + 5, MAX_N)})
    print(f"largest grid: {blocks} workgroups of {threads}, {full} words per pass; large sizes {big}")
    return host, dev, big


def sizes(vec):
    return list(SMALL) + vec[2]


def test_sizes(gpu, vec):
    host, dev, big = vec
    for n in sizes(vec):
        got, want = gpu.ctx.fingerprint(dev[:n]), fp_ref(host[:n])
        print(f"n = {n}: {got[0]:016X}{got[1]:016X}")
        assert got == want, n
    assert gpu.ctx.fingerprint(dev[:0]) == (0, 0)


def test_launch_shape(gpu, vec):
    host, dev, big = vec
    ctx = gpu.ctx
    full = ctx.fingerprint_shape(dev)[3]
    cap = full // 512
    for n in sizes(vec):
        blocks, threads, head, _ = ctx.fingerprint_shape(dev[:n])
        assert (blocks, head) == ((0, 0) if n == 0 else (max(1, min(cap, (n // 2 + 255) // 256)), 0)), n
    assert ctx.fingerprint_shape(dev[1:1001])[2] == 1         # an odd start: a scalar head
    assert ctx.fingerprint_shape(dev[: big[0]])[0] == cap     # beyond the largest grid: further passes, not more workgroups


@pytest.mark.parametrize("start", [1, 3])
def test_slices_that_are_only_8_byte_aligned(gpu, vec, start):
    host, dev, big = vec
    assert dev.data_ptr() % 16 == 0
    for n in (1, 2, 3, 64, 65, 256, 257, 1000, 1001, 65536, 65537, big[0] - 1, big[0], big[-1] - 2):
        t = dev[start:start + n]
        assert t.data_ptr() % 16 == 8 and t.numel() == n
        assert gpu.ctx.fingerprint(t) == fp_ref(host[start:start + n]), (start, n)
        assert gpu.ctx.fingerprint(t, 77) == fp_ref(host[start:start + n], 77), (start, n)


@pytest.mark.parametrize("offset", OFFSETS)
def test_offsets(gpu, vec, offset):
    host, dev, big = vec
    for n in (1, 2, 65, 1023, 65537, big[0]):
        assert gpu.ctx.fingerprint(dev[:n], offset) == fp_ref(host[:n], offset), (n, offset)
        assert gpu.ctx.fingerprint(dev[1:1 + n], offset) == fp_ref(host[1:1 + n], offset), (n, offset)


@pytest.mark.parametrize("offset", OFFSETS)
def test_special_values_count_as_their_bits(gpu, offset):
    ctx = gpu.ctx
    x = special_values()
    d = ctx.to_dev(x)
    assert np.array_equal(d.cpu().numpy().view(np.uint64), x.view(np.uint64))   # (the copy kept the NaN payload)
    want = fp_ref(x, offset)
    assert ctx.fingerprint(d, offset) == want
    assert ctx.fingerprint(d[1:], offset + 1) == fp_ref(x[1:], offset + 1)
    y = x.copy()
    y[0] = 0.0                                                                    # -0.0 -> 0.0
    assert ctx.fingerprint(ctx.to_dev(y), offset) == fp_ref(y, offset) != want


def test_concatenation_at_an_odd_split(gpu, vec):
    host, dev, big = vec
    ctx = gpu.ctx
    for n, cut, offset in ((1000, 333, 0), (65537, 4097, 2 ** 40 + 3), (big[0], big[0] // 2 + 1, 1)):
        assert cut % 2 == 1
        a, b = ctx.fingerprint(dev[:cut], offset), ctx.fingerprint(dev[cut:n], offset + cut)
        assert combine(a, b) == ctx.fingerprint(dev[:n], offset) == fp_ref(host[:n], offset), (n, cut)


def test_swapping_two_entries_changes_both_words(gpu):
    ctx = gpu.ctx
    x = data(1000)
    y = x.copy()
    y[17], y[600] = x[600], x[17]
    a, b = ctx.fingerprint(ctx.to_dev(x)), ctx.fingerprint(ctx.to_dev(y))
    assert a == fp_ref(x) and b == fp_ref(y) and a[0] != b[0] and a[1] != b[1]


def test_read_only_and_repeatable(gpu, vec):
    host, dev, big = vec
    ctx = gpu.ctx
    gen = ctx.quadrature_generation()
    n = big[-1]
    first = ctx.fingerprint(dev[:n], 3)
    assert ctx.fingerprint(dev[:n], 3) == first == fp_ref(host[:n], 3)
    assert ctx.quadrature_generation() == gen
    assert np.array_equal(dev.cpu().numpy().view(np.uint64), host.view(np.uint64))


def test_the_state_of_an_operator(gpu):
    """the vector the driver fingerprints: S of the context's own problem, and the same through the host entry"""
    from laghos_amd import host_lib
    S = gpu.test_prob.initial_state()[0]
    d = gpu.ctx.to_dev(S)
    assert gpu.ctx.fingerprint(d) == host_lib.fingerprint_host(S) == fp_ref(S)


def test_argument_refusals(gpu, vec):
    host, dev, big = vec
    ctx = gpu.ctx
    L = ctx.lib
    out = (ctypes.c_ulonglong * 2)(7, 7)
    p = ctypes.c_void_p(dev.data_ptr())
    assert L.lgh_vec_fingerprint(ctx.h, p, -1, 0, out) == 1 and b"bad argument" in L.lgh_last_error()   # LGH_ERR_ARG
    assert L.lgh_vec_fingerprint(ctx.h, None, 5, 0, out) == 1
    assert L.lgh_vec_fingerprint(None, p, 5, 0, out) == 1
    assert L.lgh_vec_fingerprint(ctx.h, p, 5, 0, None) == 1
    assert tuple(out) == (7, 7)
    assert L.lgh_vec_fingerprint(ctx.h, None, 0, 0, out) == 0 and tuple(out) == (0, 0)


def test_kernel_timer_id(gpu, vec):
    """LGH_KERNEL_FINGERPRINT (9): one sampled launch per call, none for n = 0"""
    host, dev, big = vec
    ctx = gpu.ctx
    L = ctx.lib
    from laghos_amd._lib import check
    check(L.lgh_ktime_begin(ctx.h, 9, 8))
    ctx.fingerprint(dev[:65537])
    ctx.fingerprint(dev[:0])
    ctx.fingerprint(dev[: big[0]])
    n, mean = ctypes.c_int(0), ctypes.c_double(0.0)
    check(L.lgh_ktime_end(ctx.h, ctypes.byref(n), ctypes.byref(mean)))
    assert n.value == 2 and mean.value > 0.0
