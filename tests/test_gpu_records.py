"""lgh_records_update (laghos_amd/csrc/lgh_records.hip) through Context.records_update against the numpy restatement of its table
(tests/records_ref.py): five successive updates with unequal dtr of random p, rho, e, v with the special cases planted in them -
ties, NaN samples, -0.0, a threshold hit exactly - for dim 1, 2, 3 at every size at which the kernel changes shape.

Sizes: 0 (no launch), 1 (the scalar tail alone), 2, 3, 255, 256, 257 (the edge of a workgroup's lanes: one lane takes two points),
and from lgh_records_shape the one-trip capacity C of the capped grid (every lane of the largest grid once), C - 1 (its last lane
takes the scalar tail's neighbour alone), C + 1 (a full trip and the tail) and 2 C + 3 (every lane twice, one a third time, and
the tail).  The ODD sizes are there for alignment: rec and v are column-major with n
doubles per column, so with n odd every second column starts at 8 mod 16 bytes and takes the kernel's 8-byte path while its
neighbours take the 16-byte one; test_bases_that_are_only_8_byte_aligned shifts the other columns and the inputs onto that path.

Bars (records_ref.check_block): every column but speed_max bit for bit, speed_max within 4 eps relative.  The kernel does not
look at the mesh: any small context will do."""
import ctypes

import numpy as np
import pytest

import records_ref as ref

pytestmark = pytest.mark.gpu

SMALL = (0, 1, 2, 3, 255, 256, 257)
TIMES = (0.0, 0.125, 0.1875, 0.5, 0.5625)      # unequal dtr; exact in binary, so t - t_last is the dtr the driver would form
THRESHOLD = 0.75
NFIELDS = 6                                    # p, rho, e, v0, v1, v2


@pytest.fixture(scope="module")
def gpu():
    from helpers import make_gpu
    from oracle.fem import Problem
    g = make_gpu(Problem(mesh="cube01_hex", rs=0, order_v=2, order_e=1, problem=1))
    yield g
    g.close()


@pytest.fixture(scope="module")
def shape(gpu):
    """(C, sizes from the launch shape): C = the points one trip of the largest grid takes"""
    blocks, threads, per_lane, trips = gpu.ctx.records_shape(2 ** 40)
    C = blocks * threads * per_lane
    assert threads == 256 and per_lane == 2 and trips > 1 and C <= 2 ** 22
    print(f"largest grid: {blocks} workgroups of {threads}, {per_lane} points per lane and trip, C = {C}")
    return C, (C - 1, C, C + 1, 2 * C + 3)


@pytest.fixture(scope="module")
def pool(shape):
    """one pool of random doubles per field, made once and never changed: update k of n points reads pool[f, 7 k : 7 k + n]"""
    C, big = shape
    rng = np.random.default_rng(20240607)
    P = rng.random((NFIELDS, max(big) + 7 * len(TIMES)))
    P[3:] = 2.0 * P[3:] - 1.0                  # velocities of both signs
    P.setflags(write=False)
    return P


def samples(pool, n, dim, threshold=THRESHOLD):
    """the five samples (p, rho, e, v (dim, n)) of n points with the special cases planted at eight spread points"""
    at = [(k * n) // 8 if n >= 8 else k % max(n, 1) for k in range(8)]
    out = []
    for k in range(len(TIMES)):
        f = pool[:, 7 * k:7 * k + n].copy()
        p, rho, e, v = f[0], f[1], f[2], f[3:3 + dim]
        if n:
            if k in (1, 2):
                p[at[0]] = 2.0                 # a tie: the same new maximum twice - the first time is kept
            if k == 2:
                p[at[1]] = np.nan              # a NaN sample: no extreme moves, the impulse turns NaN
                rho[at[2]] = np.nan
                v[dim - 1, at[3]] = np.nan
                e[at[3]] = np.nan
            if k == 0:
                p[at[4]] = -0.0                # -0.0 first, 0.0 next: 0.0 > -0.0 is false, p_max keeps the sign bit
                p[at[5]] = 0.0
                v[:, at[5]] = -0.0             # |v| = +0.0
                p[at[6]] = 0.25
            if k == 1:
                p[at[4]] = 0.0
                p[at[5]] = -0.0
                p[at[6]] = 0.5
            if k == 2:
                p[at[6]] = 0.25 if threshold is None else np.nextafter(threshold, 0.0)   # one ulp short: no arrival
            if k == 3:
                p[at[6]] = 0.25 if threshold is None else threshold                      # hit exactly: p >= threshold
            if k == 4:
                p[at[7]] = pool[0, 7 * 3 + at[7]]                                        # a tie with the sample before it
        out.append((p, rho, e, v))
    return out


def run(gpu, pool, n, dim, threshold=THRESHOLD, rec=None, shift=0, check_inputs=True):
    """the five updates on the GPU and in numpy, compared after each.  rec: a device tensor to work in (default: a fresh one of
    8 n); shift = 1: the inputs are handed over from an address that is 8 mod 16"""
    ctx = gpu.ctx
    rec = ctx.to_dev(np.full(8 * n, -7.0)) if rec is None else rec
    want, t_last = None, None
    for k, (p, rho, e, v) in enumerate(samples(pool, n, dim, threshold)):
        host = [p, rho, e, v.reshape(-1)]
        whole = [ctx.to_dev(np.concatenate([np.zeros(shift), a])) for a in host]
        dev = [w[shift:] for w in whole]
        assert all(d.data_ptr() % 16 == 8 * shift for d in dev if d.numel())
        t = TIMES[k]
        dtr = 0.0 if k == 0 else t - t_last
        ctx.records_update(dim, dev[0], dev[1], dev[2], dev[3], t, dtr, rec, threshold=threshold, first=(k == 0))
        ctx.sync()
        want = ref.update(want, p, rho, e, v, t, dtr, threshold, first=(k == 0))
        t_last = t
        got = rec.cpu().numpy().reshape(8, n)
        ref.check_block(got, want, dim, f"n = {n}, dim = {dim}, update {k}")
        if check_inputs and (k == len(TIMES) - 1 or n <= 257):
            for d, a in zip(dev, host):
                assert np.array_equal(ref.bits(d.cpu().numpy()), ref.bits(a))       # the inputs are read only
    return want


def check_planted(want, n, threshold):
    """the numpy result itself shows the special cases (so the comparison above checked them)"""
    at = [(k * n) // 8 for k in range(8)]
    assert want[0, at[0]] == 2.0 and want[1, at[0]] == TIMES[1]                      # the tie kept the first time
    assert np.isnan(want[2, at[1]]) and not np.isnan(want[0, at[1]])                 # NaN: impulse NaN, extremes intact
    assert not np.isnan(want[4, at[2]]) and not np.isnan(want[5, at[3]]) and not np.isnan(want[6, at[3]])
    assert want[7, at[6]] == (-1.0 if threshold is None else TIMES[3])               # arrival at the exact hit, not one ulp below
    if threshold is None:
        assert np.all(want[7] == -1.0)
    else:
        assert np.any(want[7] == -1.0) and np.any(want[7] == TIMES[0]) and np.any(want[7] == TIMES[4])


@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("n", SMALL)
def test_small_sizes(gpu, pool, n, dim):
    want = run(gpu, pool, n, dim)
    if n >= 255:
        check_planted(want, n, THRESHOLD)


@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("which", range(4))
def test_sizes_at_the_edges_of_the_grid(gpu, pool, shape, which, dim):
    C, big = shape
    n = big[which]
    blocks, threads, per_lane, trips = gpu.ctx.records_shape(n)
    assert blocks * threads * per_lane == C and trips == (1, 1, 1, 3)[which]
    check_planted(run(gpu, pool, n, dim), n, THRESHOLD)


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_no_threshold(gpu, pool, shape, dim):
    for n in (3, 257, shape[0] + 1):
        want = run(gpu, pool, n, dim, threshold=None, check_inputs=False)
        assert np.all(want[7] == -1.0)
        if n > 8:
            check_planted(want, n, None)


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_bases_that_are_only_8_byte_aligned(gpu, pool, dim):
    """rec and the inputs from addresses that are 8 mod 16: with n even every column is misaligned, with n odd the columns that
    were aligned in the tests above"""
    ctx = gpu.ctx
    for n in (2, 256, 257, 1001, 4096):
        whole = ctx.to_dev(np.full(8 * n + 2, -7.0))
        rec = whole[1:1 + 8 * n]
        assert whole.data_ptr() % 16 == 0 and rec.data_ptr() % 16 == 8
        run(gpu, pool, n, dim, rec=rec, shift=1)
        w = whole.cpu().numpy()
        assert w[0] == -7.0 and w[-1] == -7.0                                        # nothing written outside the block


def test_launch_shape(gpu, shape):
    C, big = shape
    cap = C // 512
    for n in SMALL + big:
        blocks, threads, per_lane, trips = gpu.ctx.records_shape(n)
        pairs = n // 2
        b = max(1, min(cap, (pairs + 255) // 256))
        assert (blocks, threads, per_lane, trips) == ((0, 256, 2, 0) if n == 0 else (b, 256, 2, (pairs + b * 256 - 1) // (b * 256))), n


def test_leaves_the_quadrature_data_alone(gpu, pool):
    gen = gpu.ctx.quadrature_generation()
    run(gpu, pool, 257, 3)
    assert gpu.ctx.quadrature_generation() == gen


def test_operator_samples_and_updates(gpu):
    """HydroOperator.update_records: two states, on the volume lattice and on the boundary faces, against the replay of what
    sample_fields / face_fields give for the same states"""
    from helpers import deformed_state
    from laghos_amd import host_lib
    g, ctx = gpu, gpu.ctx
    prob, R, thr = g.p, 2, 0.4                                     # p = 0.4 rho e with rho near 1 and e in 0.5 .. 1.5: some points reach it
    dim = prob.dim
    faces = ctx.boundary_faces()
    n_f, n_v = len(faces) * (R + 1) ** (dim - 1), prob.NE * (R + 1) ** dim
    rec_f, rec_v = ctx.to_dev(np.full(8 * n_f, -7.0)), ctx.to_dev(np.full(8 * n_v, -7.0))
    Bh, Bl = host_lib.host_lattice_tables(prob.order_v, prob.order_e, R)
    want_f = want_v = None
    for k, t in enumerate((0.0, 0.25, 0.3125)):
        S = ctx.to_dev(deformed_state(prob, seed=3 + k))
        dtr = 0.0 if k == 0 else t - (0.0, 0.25)[k - 1]
        assert g.update_records(S, R, rec_f, t, dtr=dtr, threshold=thr, first=(k == 0), faces=faces) == n_f
        assert g.update_records(S, R, rec_v, t, dtr=dtr, threshold=thr, first=(k == 0)) == n_v
        d = g.face_fields(S, R, faces, fields=("p", "rho", "e", "v"))
        want_f = ref.update(want_f, d["p"], d["rho"], d["e"], d["v"], t, dtr, thr, first=(k == 0))
        f = dict(v=ctx.empty(dim * n_v), e=ctx.empty(n_v), rho=ctx.empty(n_v), p=ctx.empty(n_v))
        ctx.sample_fields(S, g.compute_density(S), Bh, Bl, **f)
        ctx.sync()
        h = {key: a.cpu().numpy() for key, a in f.items()}
        want_v = ref.update(want_v, h["p"], h["rho"], h["e"], h["v"].reshape(dim, n_v), t, dtr, thr, first=(k == 0))
        ref.check_block(rec_f.cpu().numpy().reshape(8, n_f), want_f, dim, f"faces, update {k}")
        ref.check_block(rec_v.cpu().numpy().reshape(8, n_v), want_v, dim, f"volume, update {k}")
    assert np.any(want_v[7] >= 0.0) and np.any(want_v[1] > 0.0)


def test_argument_refusals(gpu, pool):
    """every refusal: LGH_ERR_ARG, a message naming the value, and rec keeps its bits"""
    ctx = gpu.ctx
    L = ctx.lib
    n = 257
    p, rho, e, v = (ctx.to_dev(a.reshape(-1)) for a in samples(pool, n, 3)[0])
    start = np.full(8 * n, -7.0)
    rec = ctx.to_dev(start)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    nan, inf = float("nan"), float("inf")

    def call(n=n, dim=3, p=P(p), rho=P(rho), e=P(e), v=P(v), t=1.0, dtr=0.5, thr=nan, first=0, rec=P(rec)):
        return L.lgh_records_update(ctx.h, n, dim, p, rho, e, v, t, dtr, thr, first, rec), L.lgh_last_error().decode()

    cases = {
        "n < 0": (dict(n=-3), "-3"),
        "p NULL": (dict(p=None), "p is NULL"),
        "rho NULL": (dict(rho=None), "rho is NULL"),
        "e NULL": (dict(e=None), "e is NULL"),
        "v NULL": (dict(v=None), "v is NULL"),
        "rec NULL": (dict(rec=None), "rec is NULL"),
        "dim 0": (dict(dim=0), "dim = 0"),
        "dim 4": (dict(dim=4), "dim = 4"),
        "t NaN": (dict(t=nan), "nan"),
        "t inf": (dict(t=inf), "inf"),
        "dtr < 0": (dict(dtr=-0.25), "-0.25"),
        "dtr NaN": (dict(dtr=nan), "nan"),
        "dtr inf": (dict(dtr=inf), "inf"),
        "first with dtr": (dict(first=1, dtr=0.5), "0.5"),
        "threshold inf": (dict(thr=inf), "inf"),
        "threshold -inf": (dict(thr=-inf), "-inf"),
    }
    for name, (kw, word) in cases.items():
        rc, msg = call(**kw)
        assert rc == 1 and "lgh_records_update" in msg and word in msg, (name, rc, msg)      # LGH_ERR_ARG
    ctx.sync()
    assert np.array_equal(ref.bits(rec.cpu().numpy()), ref.bits(start))
    assert call(n=0, p=None, rho=None, e=None, v=None, rec=None)[0] == 0                      # n == 0: LGH_OK, nothing to read
    ctx.sync()
    assert np.array_equal(ref.bits(rec.cpu().numpy()), ref.bits(start))


def test_kernel_timer_id(gpu, pool):
    """LGH_KERNEL_RECORDS (17): one sampled launch per call, none for n = 0"""
    ctx = gpu.ctx
    L = ctx.lib
    from laghos_amd._lib import check
    check(L.lgh_ktime_begin(ctx.h, 17, 32))
    run(gpu, pool, 0, 3, check_inputs=False)
    run(gpu, pool, 1001, 2, check_inputs=False)
    n, mean = ctypes.c_int(0), ctypes.c_double(0.0)
    check(L.lgh_ktime_end(ctx.h, ctypes.byref(n), ctypes.byref(mean)))
    assert n.value == len(TIMES) and mean.value > 0.0
