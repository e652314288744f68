"""The host side of the exchanges (lgh_comm.hip, lgh_comm_transport.hip) at its edges: neighbour tables replaced on a live
context, refused calls, the in-process transport on all-pairs and other partitions, peers whose lists disagree.  Every case
runs on the smallest block with the structure (cube01_hex, rs=1, Q2Q1, one rank of 2 x 2 x 2: 8 zones, 125 nodes - as test_halo_logic_emulated_ranks
of tests/test_gpu_pipeline.py, whose emulated ranks and layout model it shares) and compares bit for bit with a numpy model:

    block of neighbour k at base_k = 3 * off_k + 4 * k, component-major: buf[base_k + c * cnt_k + i] = v[c * N + node_k[i]];
    a shared node becomes the sum of its copies in ascending rank order, the own value at this rank's position."""
import ctypes

import numpy as np
import pytest

from rank_threads import local_unique_id, run_ranks

pytestmark = pytest.mark.gpu

LGH_ERR_ARG, LGH_ERR_COMM = 1, 4
ROOM = 2048            # doubles in every buffer the test hands to lgh_test_halo_pack / _combine: more than any table here needs
MARK = -7.25e300       # what the room behind a buffer must still hold afterwards


def _context():
    from laghos_amd.context import Context
    from oracle.fem import Problem
    # (the block of one rank of the 2 x 2 x 2 partition: 8 zones, 125 nodes)
    p = Problem(mesh="cube01_hex", rs=1, order_v=2, order_e=1, problem=1, rank=0, pgrid=[2, 2, 2])
    assert (p.NE, p.N) == (8, 125)
    _, _, gamma, _ = p.initial_state()
    c = Context(p.dim, p.NE, p.D1D, p.Q1D, p.L1D, p.N, p.h1map, p.B, p.G, p.Bl, p.W, gamma, p.ess, order_v=p.order_v)
    return p, c


def _layout(lists):
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(int)
    base = [3 * int(off[k]) + 4 * k for k in range(len(lists))]
    return off, base, 3 * max(int(off[-1]), 1) + 4 * len(lists)


def _ordered_sum(vals):
    s = np.float64(vals[0])
    for x in vals[1:]:
        s = s + np.float64(x)
    return s


def _combine_model(N, rank, ranks, lists, own, recv, ncomp):
    """own (ncomp * N) with every shared node replaced by the rank-ordered sum of its copies; recv: a receive buffer"""
    off, base, _ = _layout(lists)
    out = own.copy()
    copies = {}   # node -> [(rank, entry of the concatenated lists, neighbour, position in its list)]
    for k, l in enumerate(lists):
        for i, n in enumerate(l):
            copies.setdefault(int(n), [(rank, -1, -1, -1)]).append((ranks[k], int(off[k]) + i, k, i))
    for n, src in copies.items():
        for c in range(ncomp):
            vals = [own[c * N + n] if k < 0 else recv[base[k] + c * len(lists[k]) + i] for _, _, k, i in sorted(src)]
            out[c * N + n] = _ordered_sum(vals)
    return out, len(copies)


def _stats(c):
    nn, mx, sh, ap, c2 = ctypes.c_int(), ctypes.c_long(), ctypes.c_long(), ctypes.c_int(), ctypes.c_int()
    assert c.lib.lgh_comm_stats(c.h, ctypes.byref(nn), ctypes.byref(mx), ctypes.byref(sh), ctypes.byref(ap), ctypes.byref(c2)) == 0
    return nn.value, mx.value, sh.value, ap.value, c2.value


def _check_tables(c, N, rank, ranks, lists, rng):
    """pack and combine with ncomp = 1, 2, 3 and lgh_comm_stats answer for exactly these lists"""
    import torch
    off, base, size = _layout(lists)
    assert size <= ROOM
    v = rng.standard_normal(3 * N) * 10.0 ** rng.integers(-8, 9, 3 * N)
    recv = np.full(ROOM, MARK)
    recv[:size] = rng.standard_normal(size) * 10.0 ** rng.integers(-8, 9, size)
    vd, rd = c.to_dev(v), c.to_dev(recv)
    n_shared = 0
    for ncomp in (1, 2, 3):
        out = c.to_dev(np.full(ROOM, MARK))
        c.test_halo_pack(vd, ncomp, out)
        c.sync()
        got = out.cpu().numpy()
        assert np.all(got[size:] == MARK) and not np.any(got[:size] == MARK), "the send buffer has another size"
        for k, l in enumerate(lists):
            for cc in range(ncomp):
                want = v[cc * N + np.asarray(l, dtype=int)]
                assert np.array_equal(got[base[k] + cc * len(l): base[k] + (cc + 1) * len(l)], want), (ncomp, k, cc)
        own = c.clone(vd)
        c.test_halo_combine(rd, own, ncomp)
        c.sync()
        torch.cuda.synchronize()
        want, n_shared = _combine_model(N, rank, ranks, lists, v, recv, ncomp)
        assert np.array_equal(own.cpu().numpy()[:ncomp * N], want[:ncomp * N]), ncomp
        assert np.array_equal(own.cpu().numpy()[ncomp * N:], v[ncomp * N:]), ncomp
    assert _stats(c)[:3] == (len(lists), max(len(l) for l in lists), n_shared)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


# seven neighbours of rank 3 of 8, three nodes each but for one empty list; nodes 7, 11 and 40 are listed under several
SEVEN_RANKS = [0, 1, 2, 4, 5, 6, 7]
SEVEN_LISTS = [_i32([7, 11, 40]), _i32([11, 12, 13]), _i32([]), _i32([40, 7, 99]), _i32([124, 0, 11]), _i32([60, 61, 62]), _i32([7, 63, 64])]
ONE_LIST = [_i32([3, 30, 31, 77, 124])]


def test_repartition_on_one_context():
    """lgh_test_set_rank + lgh_comm_set_neighbors three times on one context: after each call the tables are those of that
    call alone - layout, rank-ordered combine (own value in the middle of the ranks, nodes under several neighbours, an empty
    list) and the counts lgh_comm_stats reports."""
    p, c = _context()
    rng = np.random.default_rng(11)
    try:
        for nranks, rank, ranks, lists in ((2, 0, [1], ONE_LIST), (8, 3, SEVEN_RANKS, SEVEN_LISTS), (2, 1, [0], ONE_LIST)):
            c.test_set_rank(nranks, rank)
            c.comm_set_neighbors(ranks, lists)
            _check_tables(c, p.N, rank, ranks, lists, rng)
            assert _stats(c)[3:] == (1, 0)   # every other rank is a neighbour; no communicator, no second channel
    finally:
        c.close()


def _set_neighbors_raw(c, ranks, counts, lists):
    ip = ctypes.POINTER(ctypes.c_int)
    n = len(ranks)
    r, k = _i32(ranks if n else [0]), _i32(counts if n else [0])
    keep = [_i32(l if len(l) else [0]) for l in lists] or [_i32([0])]
    arr = (ip * len(keep))(*[l.ctypes.data_as(ip) for l in keep])
    return c.lib.lgh_comm_set_neighbors(c.h, n, r.ctypes.data_as(ip), k.ctypes.data_as(ip), arr)


def test_refused_calls_leave_the_previous_tables_in_force():
    p, c = _context()
    rng = np.random.default_rng(12)
    try:
        c.test_set_rank(2, 0)
        c.comm_set_neighbors([1], ONE_LIST)
        _check_tables(c, p.N, 0, [1], ONE_LIST, rng)
        refused = (([1], [3], [[3, p.N, 5]]),            # a node index N
                   ([1], [-1], [[3]]),                   # a negative count
                   ([], [], []))                         # no neighbour on a communicator of two
        for ranks, counts, lists in refused:
            assert _set_neighbors_raw(c, ranks, counts, lists) == LGH_ERR_ARG, (ranks, counts)
            _check_tables(c, p.N, 0, [1], ONE_LIST, rng)
            assert _stats(c)[3:] == (1, 0)
    finally:
        c.close()


def _row_lists(p, nr, r):
    """nr cubes in a row along x: the face x = max of rank r is the face x = min of rank r + 1 (nodes in the same (z, y) order)"""
    X = p.node_coords()
    face = lambda x: np.array(sorted(np.flatnonzero(X[0] == x), key=lambda n: (X[2][n], X[1][n])), dtype=np.int32)
    lo, hi = face(X[0].min()), face(X[0].max())
    assert len(lo) == len(hi) == 25
    ranks, lists = [], []
    if r > 0:
        ranks.append(r - 1); lists.append(lo)
    if r + 1 < nr:
        ranks.append(r + 1); lists.append(hi)
    return ranks, lists


@pytest.mark.parametrize("piggyback", ["1", "0"])
@pytest.mark.parametrize("nr", [2, 3])
def test_in_process_transport_rows_of_ranks(nr, piggyback, monkeypatch):
    """Two cubes in a row are an all-pairs partition, three are not (the middle rank alone sees both others): lgh_halo_sum
    and lgh_allreduce over the in-process transport, with and without the sums that ride on the halo messages."""
    monkeypatch.setenv("LGH_HALO_PIGGYBACK", piggyback)
    cid = local_unique_id()
    f = lambda X, r: (np.sin(3 * (X[0] + r)) * np.cos(2 * X[1]) + X[2] ** 2) * 10.0 ** (3 * r)
    red = [1e16, 1.0, -1e16][:nr]   # (1e16 + 1) - 1e16 = 0 in rank order, 1 in any other
    ctxs = [None] * nr

    def rank_main(r):
        p, c = _context()
        ctxs[r] = c
        c.comm_init(nr, r, cid)
        ranks, lists = _row_lists(p, nr, r)
        c.comm_set_neighbors(ranks, lists)
        v = np.concatenate([f(p.node_coords(), r) * (1 + cc) for cc in range(3)])
        sums = {}
        for ncomp in (1, 3):
            vd = c.to_dev(v)
            c.halo_sum(vd, ncomp)
            c.sync()
            sums[ncomp] = vd.cpu().numpy()
        return dict(N=p.N, v=v, sums=sums, lists=dict(zip(ranks, lists)), stats=_stats(c),
                    total=c.allreduce(red[r], 0), least=c.allreduce(red[r], 1))

    try:
        out = run_ranks(nr, rank_main)
    finally:
        for c in ctxs:
            if c is not None:
                c.close()
    for r, o in enumerate(out):
        N = o["N"]
        assert o["stats"] == (len(o["lists"]), 25, 25 * len(o["lists"]), 1 if nr == 2 else 0, 1), (r, o["stats"])
        assert o["total"] == _ordered_sum(red) and o["least"] == min(red), (r, o["total"], o["least"])
        for ncomp in (1, 3):
            want = o["v"].copy()
            for peer, l in o["lists"].items():
                mine, theirs = o["v"], out[peer]["v"]
                l_peer = out[peer]["lists"][r]
                for cc in range(ncomp):
                    a, b = mine[cc * N + l], theirs[cc * N + l_peer]
                    want[cc * N + l] = (a + b) if r < peer else (b + a)
                    # every copy of a shared node holds the same bits
                    assert np.array_equal(o["sums"][ncomp][cc * N + l], out[peer]["sums"][ncomp][cc * N + l_peer]), (r, peer, ncomp)
            assert np.array_equal(o["sums"][ncomp][:ncomp * N], want[:ncomp * N]), (r, ncomp)
            assert np.array_equal(o["sums"][ncomp][ncomp * N:], o["v"][ncomp * N:]), (r, ncomp)


def test_neighbour_counts_that_disagree():
    """Two ranks whose lists for each other have 5 and 4 nodes: both find it at the same point of lgh_halo_sum, so neither
    waits for the other, and both return LGH_ERR_COMM with a message."""
    cid = local_unique_id()
    ctxs = [None, None]

    def rank_main(r):
        p, c = _context()
        ctxs[r] = c
        c.comm_init(2, r, cid)
        c.comm_set_neighbors([1 - r], [ONE_LIST[0][:5 - r]])
        v = c.zeros(p.N)
        rc = c.lib.lgh_halo_sum(c.h, ctypes.c_void_p(v.data_ptr()), 1)
        return rc, c.lib.lgh_last_error().decode()

    try:
        out = run_ranks(2, rank_main)
    finally:
        for c in ctxs:
            if c is not None:
                c.close()
    for rc, msg in out:
        assert rc == LGH_ERR_COMM and "do not match" in msg, (rc, msg)
