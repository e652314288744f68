"""The conditions the several-rank GPU tests (tests/test_gpu_ranks_2d.py, tests/test_gpu_ranks_3d.py, the 2D entries of
tests/test_gpu_pipeline.py::MULTI_RANK_CASES) rely on, checked on the oracle and the host library alone - no GPU."""
import numpy as np
import pytest

import rank_cases as rc
import shape_cases as sc
from laghos_amd import host_lib

GRIDS = list(rc.RANK_GRIDS)
ids = [rc.grid_id(g) for g in GRIDS]


@pytest.mark.parametrize("pgrid", GRIDS, ids=ids)
def test_partition_picks_the_rank_grid_of_the_table(pgrid):
    """laghos::Partition, given the global zone grid and the rank count, picks exactly the rank grid of the table - so the
    C++ driver's run of `-nx -ny` on that many ranks is the partition the kernel-level tests build with the oracle"""
    shape = rc.global_shape(pgrid)
    assert shape == (13 * pgrid[0], 5 * pgrid[1])
    assert host_lib.host_partition(2, shape[0], shape[1], 1, rc.n_ranks(pgrid))[:2] == tuple(pgrid)


def test_partition_of_the_other_whole_runs():
    """The grids that are not in the table.  Problem 3 runs on the 7 x 3 box (interfaces at x = 1 and y = 1.5): 28 x 12 zones
    on four ranks are split 4 x 1 by laghos::Partition (28 -> 14 -> 7: the axis with the most local zones is halved), a chain
    of four in which all three materials cross the boundaries between the ranks; 28 x 16 zones are split 2 x 2, the
    interface at y = 1.5 on the boundary between the rank rows, the one at x = 1 at zone 4 of the left column.  And the 3D
    block pair."""
    assert host_lib.host_partition(2, 28, 12, 1, 4)[:2] == (4, 1)
    assert host_lib.host_partition(2, 28, 16, 1, 4)[:2] == (2, 2)
    assert host_lib.host_partition(3, 10, 3, 2, 2) == rc.GRID_3D


@pytest.mark.parametrize("pgrid", GRIDS, ids=ids)
@pytest.mark.parametrize("mesh", rc.MESHES)
def test_blocks_neighbours_and_owners(pgrid, mesh):
    glob, ranks = rc.problems(pgrid, mesh, (3, 2))
    assert len(ranks) == rc.n_ranks(pgrid)
    for p in ranks:
        assert (tuple(p.ne), p.NE, p.N) == (rc.BLOCK, 65, 640)   # 3 workgroups of cg_init_k, 2 of cg_update_k
    assert 65 % 16 and 65 % 7 and 65 % 4                          # ragged against the 2D batches of Q2Q1, Q3Q2, Q4Q3
    # the maps from integer block offsets name the same physical nodes and zones
    X, V = glob.node_coords(), glob.elem_volumes()
    for p in ranks:
        assert np.array_equal(X[:, rc.node_map(p)], p.node_coords())
        assert np.array_equal(V[rc.zone_map(p)], p.elem_volumes())
        assert np.array_equal(np.asarray(glob.h1map)[rc.zone_map(p)], rc.node_map(p)[np.asarray(p.h1map)])
    # every global node is owned exactly once
    owned = np.zeros(glob.N)
    for p in ranks:
        assert set(np.unique(p.owner)) <= {0.0, 1.0}
        np.add.at(owned, rc.node_map(p), p.owner)
    assert np.array_equal(owned, np.ones(glob.N))
    # neighbour lists: symmetric, the same global nodes in the same order on both sides, the peer counts of the table
    nbrs = [p.neighbors() for p in ranks]
    assert [len(n[0]) for n in nbrs] == rc.PEERS[pgrid]
    held = np.zeros(glob.N, dtype=int)
    for p in ranks:
        held[rc.node_map(p)] += 1
    for r, (p, (nr, lists)) in enumerate(zip(ranks, nbrs)):
        assert len(set(nr)) == len(nr) and r not in nr
        shared = np.zeros(p.N, dtype=int)
        for peer, mine in zip(nr, lists):
            pr, pl = nbrs[peer]
            assert list(pr).count(r) == 1
            theirs = pl[list(pr).index(r)]
            assert len(mine) == len(theirs) > 0
            assert np.array_equal(rc.node_map(p)[mine], rc.node_map(ranks[peer])[theirs])
            shared[mine] += 1
        assert np.array_equal(shared + 1, held[rc.node_map(p)])   # every other holder of a node is a peer that lists it
    if pgrid[0] > 1 and pgrid[1] > 1:
        assert held.max() == 4          # a corner node held by four ranks
    else:
        assert held.max() == 2
    all_pairs = all(len(n[0]) == len(ranks) - 1 for n in nbrs)
    assert all_pairs == (pgrid in ((2, 1), (1, 2), (2, 2)))


@pytest.mark.parametrize("pgrid", GRIDS + [rc.GRID_3D], ids=ids + ["2x1x1ranks"])
def test_graded_meshes_keep_distinct_volumes(pgrid):
    """every zone its own mass factor: all zone volumes pairwise distinct by more than 1e-6 relative, neighbouring widths
    along an axis by more than 2e-3, widths within +-30 % of the axis mean, hx != hy (!= hz) in every zone; the equal mesh
    is the driver's (rank_cases.py says why the bound of shape_cases cannot hold for 130 zones and more)"""
    shape = rc.global_shape(pgrid)
    order = (3, 2) if len(pgrid) == 2 else rc.ORDER_3D
    glob, ranks = rc.problems(pgrid, "graded", order)
    rc.check_graded(glob)
    v = np.sort(glob.elem_volumes())
    assert np.min(np.diff(v) / v[1:]) > 1e-6 * (1 - 1e-9)
    for a, n in enumerate(shape):
        w = np.diff(glob.gbreaks[a])
        assert np.all(np.abs(w * n / sc.AXIS_LENGTHS[a] - 1.0) <= 0.30)
        assert glob.gbreaks[a][0] == 0.0 and glob.gbreaks[a][-1] == sc.AXIS_LENGTHS[a]
    eq = rc.breaks(shape, "equal")
    for a, n in enumerate(shape):
        assert np.array_equal(eq[a], np.array([sc.AXIS_LENGTHS[a] * i / n for i in range(n + 1)]))


def test_3d_block_pair():
    glob, ranks = rc.problems(rc.GRID_3D, "graded", rc.ORDER_3D)
    assert [tuple(p.ne) for p in ranks] == [rc.BLOCK_3D] * 2
    assert sum(int(p.owner.sum()) for p in ranks) == glob.N
    X = glob.node_coords()
    for p in ranks:
        assert np.array_equal(X[:, rc.node_map(p)], p.node_coords())


def test_slices_and_gathers_are_inverse():
    glob, ranks = rc.problems((3, 2), "graded", (3, 2))
    rng = np.random.default_rng(5)
    S = rng.uniform(-1, 1, 2 * glob.H1V + glob.L2V)
    pieces = [rc.slice_state(p, S) for p in ranks]
    for k in range(2):
        back = rc.gather_nodes(ranks, [s[k * p.H1V:(k + 1) * p.H1V] for p, s in zip(ranks, pieces)], 2)
        assert np.array_equal(back, S[k * glob.H1V:(k + 1) * glob.H1V])
    assert np.array_equal(rc.gather_zones(ranks, [s[2 * p.H1V:] for p, s in zip(ranks, pieces)], glob.NL), S[2 * glob.H1V:])
    sJ = rng.uniform(-1, 1, 4 * glob.NE * glob.NQ)
    for p in ranks:
        got = rc.slice_stress(p, sJ).reshape(4, p.NE, p.NQ)
        assert np.array_equal(got[3, 7], sJ.reshape(4, glob.NE, glob.NQ)[3, rc.zone_map(p)[7]])
    # a copy of a shared node that differs in one bit is caught
    bad = [s[:p.N].copy() for p, s in zip(ranks, pieces)]
    bad[1][0] = np.nextafter(bad[1][0], 2.0)   # node 0 of rank 1 lies on rank 0's edge
    with pytest.raises(AssertionError):
        rc.gather_nodes(ranks, bad, 1)


# ---- the 3D table (tests/test_gpu_ranks_3d.py) ---------------------------------------------------------------------------------
GRIDS_3D = list(rc.RANK_GRIDS_3D)
ids_3d = [rc.grid_id(g) for g in GRIDS_3D]


def test_3d_table_is_the_issue_s():
    assert GRIDS_3D == [(2, 1, 1), (1, 1, 2), (2, 2, 2), (3, 1, 1), (3, 3, 1)]
    assert [rc.global_shape(g) for g in GRIDS_3D] == [(10, 3, 2), (5, 3, 4), (10, 6, 4), (15, 2, 2), (15, 6, 2)]
    assert max(rc.n_ranks(g) for g in GRIDS_3D) == 9                      # nine contexts at most at a time
    assert rc.global_shape(rc.GRID_3D) == (10, 3, 2) and rc.block_of(rc.GRID_3D) == rc.BLOCK_3D   # the 2D module's 3D case
    assert rc.global_shape((2, 2, 1)) == (10, 6, 2)                       # a 3D grid outside the table: BLOCK_3D (problem 7)
    assert rc.global_shape((3, 2)) == (39, 10)                            # 2D as before
    for n in (30, 20):                                                    # ragged against the plane, column and Kronecker batches
        assert n % 13 and n % 7 and n % 16
    assert 30 % sc.ES == 0 and sc.n_chains((5, 3, 2)) == 6 and sc.n_chains((5, 2, 2)) == 4   # full slab sets, each an x-chain


@pytest.mark.parametrize("pgrid", GRIDS_3D + [(2, 2, 1)], ids=ids_3d + ["2x2x1ranks"])
def test_partition_picks_the_3d_rank_grid(pgrid):
    """laghos::Partition on the global zone grid and the rank count picks the rank grid the kernel-level tests build with the
    oracle - all five of the table, and 2 x 2 x 1 for the problem-7 case"""
    shape = rc.global_shape(pgrid)
    assert host_lib.host_partition(3, shape[0], shape[1], shape[2], rc.n_ranks(pgrid)) == tuple(pgrid)


@pytest.mark.parametrize("pgrid", GRIDS_3D, ids=ids_3d)
@pytest.mark.parametrize("mesh", rc.MESHES)
def test_blocks_neighbours_and_owners_3d(pgrid, mesh):
    glob, ranks = rc.problems(pgrid, mesh, (3, 2))
    block = rc.RANK_GRIDS_3D[pgrid][0]
    NE, N = int(np.prod(block)), int(np.prod([3 * b + 1 for b in block]))
    assert (NE, N) in ((30, 1120), (20, 784))
    assert len(ranks) == rc.n_ranks(pgrid) and glob.N <= 7657 and glob.NE <= 240
    for p in ranks:
        assert (tuple(p.ne), p.NE, p.N) == (block, NE, N)
    # the maps from integer block offsets name the same physical nodes and zones
    X, V = glob.node_coords(), glob.elem_volumes()
    for p in ranks:
        assert np.array_equal(X[:, rc.node_map(p)], p.node_coords())
        assert np.array_equal(V[rc.zone_map(p)], p.elem_volumes())
        assert np.array_equal(np.asarray(glob.h1map)[rc.zone_map(p)], rc.node_map(p)[np.asarray(p.h1map)])
    # every global node is owned exactly once
    owned = np.zeros(glob.N)
    for p in ranks:
        assert set(np.unique(p.owner)) <= {0.0, 1.0}
        np.add.at(owned, rc.node_map(p), p.owner)
    assert np.array_equal(owned, np.ones(glob.N))
    # neighbour lists: symmetric, the same global nodes in the same order on both sides, in ascending rank order (the
    # lockstep energy solve folds its sums in that order: comm_ranks_before), the peer counts of the table
    nbrs = [p.neighbors() for p in ranks]
    assert [len(n[0]) for n in nbrs] == rc.PEERS_3D[pgrid]
    held = np.zeros(glob.N, dtype=int)
    for p in ranks:
        held[rc.node_map(p)] += 1
    for r, (p, (nr, lists)) in enumerate(zip(ranks, nbrs)):
        assert list(nr) == sorted(set(nr)) and r not in nr
        shared = np.zeros(p.N, dtype=int)
        for peer, mine in zip(nr, lists):
            pr, pl = nbrs[peer]
            assert list(pr).count(r) == 1
            theirs = pl[list(pr).index(r)]
            assert len(mine) == len(theirs) > 0
            assert np.array_equal(rc.node_map(p)[mine], rc.node_map(ranks[peer])[theirs])
            shared[mine] += 1
        assert np.array_equal(shared + 1, held[rc.node_map(p)])   # every other holder of a node is a peer that lists it
    assert held.max() == rc.HELD_MAX_3D[pgrid]
    all_pairs = all(len(n[0]) == len(ranks) - 1 for n in nbrs)
    assert all_pairs == rc.ALL_PAIRS_3D[pgrid]


@pytest.mark.parametrize("pgrid", GRIDS_3D, ids=ids_3d)
def test_graded_meshes_keep_distinct_volumes_3d(pgrid):
    """the conditions of test_graded_meshes_keep_distinct_volumes on the 3D table, at Q3Q2, on the global problem and on
    every rank's block"""
    shape = rc.global_shape(pgrid)
    glob, ranks = rc.problems(pgrid, "graded", (3, 2))
    rc.check_graded(glob)
    for p in ranks:
        rc.check_graded(p)
    v = np.sort(glob.elem_volumes())
    assert np.min(np.diff(v) / v[1:]) > 1e-6 * (1 - 1e-9)
    for a, n in enumerate(shape):
        w = np.diff(glob.gbreaks[a])
        assert np.all(np.abs(np.diff(w)) > 2e-3 * w[1:] * (1 - 1e-9))
        assert np.all(np.abs(w * n / sc.AXIS_LENGTHS[a] - 1.0) <= 0.30)
        assert glob.gbreaks[a][0] == 0.0 and glob.gbreaks[a][-1] == sc.AXIS_LENGTHS[a]
    eq = rc.breaks(shape, "equal")
    for a, n in enumerate(shape):
        assert np.array_equal(eq[a], np.array([sc.AXIS_LENGTHS[a] * i / n for i in range(n + 1)]))


def test_slices_and_gathers_are_inverse_3d():
    glob, ranks = rc.problems((2, 2, 2), "graded", (3, 2))
    rng = np.random.default_rng(5)
    S = rng.uniform(-1, 1, 2 * glob.H1V + glob.L2V)
    pieces = [rc.slice_state(p, S) for p in ranks]
    for k in range(2):
        back = rc.gather_nodes(ranks, [s[k * p.H1V:(k + 1) * p.H1V] for p, s in zip(ranks, pieces)], 3)
        assert np.array_equal(back, S[k * glob.H1V:(k + 1) * glob.H1V])
    assert np.array_equal(rc.gather_zones(ranks, [s[2 * p.H1V:] for p, s in zip(ranks, pieces)], glob.NL), S[2 * glob.H1V:])
    sJ = rng.uniform(-1, 1, 9 * glob.NE * glob.NQ)
    for p in ranks:
        got = rc.slice_stress(p, sJ).reshape(9, p.NE, p.NQ)
        assert np.array_equal(got[7, 11], sJ.reshape(9, glob.NE, glob.NQ)[7, rc.zone_map(p)[11]])
    # a copy of the corner node (held by all eight ranks) that differs in one bit on the last rank is caught
    bad = [s[:p.N].copy() for p, s in zip(ranks, pieces)]
    bad[7][0] = np.nextafter(bad[7][0], 2.0)
    with pytest.raises(AssertionError):
        rc.gather_nodes(ranks, bad, 1)


def test_permuted_rank_translates_the_neighbour_lists():
    """rank_cases.permuted_rank: both sides of every pair still list the same global nodes in the same order, the owner
    weights and essential rows follow the nodes, and a result comes back to the generator's numbering"""
    glob, ranks = rc.problems((2, 2, 2), "graded", (3, 2))
    perms = [rc.permuted_rank(p, seed=31 + p.rank) for p in ranks]
    gmap = []
    for p, q in zip(ranks, perms):
        m = np.empty(p.N, dtype=np.int64)
        m[q.node_perm] = rc.node_map(p)          # global node of every node of the new numbering
        gmap.append(m)
        assert not np.array_equal(q.node_perm, np.arange(p.N))
        assert np.array_equal(q.owner[q.node_perm], p.owner)
        for a in range(3):
            assert np.array_equal(np.sort(gmap[-1][q.ess[a]]), np.sort(rc.node_map(p)[p.ess[a]]))
        v = np.random.default_rng(p.rank).uniform(-1, 1, 3 * p.N)
        assert np.array_equal(rc.unpermute_nodes(q, q.nodes(v), 3), v)
        z = np.random.default_rng(p.rank).uniform(-1, 1, p.L2V)
        assert np.array_equal(rc.unpermute_zones(q, q.zones(z, p.NL), p.NL), z)
    nbrs = [q.neighbors() for q in perms]
    for r, (nr, lists) in enumerate(nbrs):
        assert list(nr) == list(ranks[r].neighbors()[0])
        for peer, mine in zip(nr, lists):
            pr, pl = nbrs[peer]
            assert np.array_equal(gmap[r][mine], gmap[peer][pl[list(pr).index(r)]])
