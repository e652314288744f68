"""Runs on several ranks: the rank grids and the element grids that go with them, shared by tests/test_rank_cases.py
(CPU: the conditions the GPU tests rely on), tests/test_gpu_ranks_2d.py and tests/test_gpu_ranks_3d.py (the kernels on
ranks), tests/test_host_setup.py and the 2D entries of tests/test_gpu_pipeline.py::MULTI_RANK_CASES.  2D first, the 3D table
at the end.

In 3D every velocity solve goes through the lockstep solver (lgh_vcg.hip); in 2D vcg_available() is false and
lgh_solve_velocity runs the scalar cg_solve(LGH_SPACE_H1) of lgh_scg.hip once per component - whose several-rank branch
(rank-summed (r, z) and (d, A d), looked at by the NEXT kernel of the sequence) no 3D run reaches.

Every rank holds a block of 13 x 5 zones.  65 is ragged against the 2D batches of 16, 7 and 4 zones (Q2Q1, Q3Q2, Q4Q3);
at Q3Q2 a block has 40 x 16 = 640 nodes: three workgroups of cg_init_k (256 nodes each) and two of cg_update_k (512), so the
ticketed grid sums cross workgroups.

  rank grid  global zones  the smallest case of
  2 x 1      26 x 5        one shared edge, all-pairs
  1 x 2      13 x 10       the shared edge along x: contiguous node lists
  2 x 2      26 x 10       a corner node held by four ranks, three peers each, all-pairs
  3 x 1      39 x 5        not all-pairs: only the middle rank sees everyone
  3 x 2      39 x 10       edge ranks with corner peers (3 and 5 peers), not all-pairs
  3 x 3      39 x 15       a middle rank with eight neighbours

Two meshes per grid:
  equal   shape_cases.breaks(shape, "equal"): what the C++ driver's -nx/-ny -Sx/-Sy builds, break for break;
  graded  the recipe of shape_cases.breaks(shape, "graded") - axis lengths 1.0 and 1.25, widths mean * (1 + 0.25 u) from a
          seed that is a fixed function of the shape, within +-30 % of the axis mean - under a distinctness condition these
          grids can meet.  shape_cases asks for zone volumes pairwise distinct by 2e-3 relative; n volumes spread over a
          factor of about 3 have a smallest gap of order 1 / n^2, so no draw of 130 to 585 zones passes it (all 1000 draws
          fail).  Here: every pair of zones differs by more than 1e-6 in volume (seven orders above the 1e-13 the
          operators are held to: a kernel that reads ANY other zone's factor is caught), and neighbouring widths along
          each axis differ by more than 2e-3 (a kernel that reads a face or corner neighbour's factor is wrong by that
          much).  hx != hy in every zone as in shape_cases.

The 3D block of the one 3D case of the 2D module (the several-rank branch of mass_apply_3d in MODE 2 is reachable through
lgh_cg_solve only): 2 x 1 x 1 ranks of 5 x 3 x 2 zones at Q2Q1.

The 3D table (tests/test_gpu_ranks_3d.py: the lockstep velocity solve of lgh_vcg.hip in its several-rank mode).  A block has 30
zones (5 x 3 x 2: six full slab sets of 5, 1120 nodes at Q3Q2) or 20 zones (5 x 2 x 2, 784 nodes), both ragged against the plane
batch of 13, the column batch of 7 and the Kronecker batch of 16:

  rank grid  block      global      the smallest case of
  2 x 1 x 1  5 x 3 x 2  10 x 3 x 2  one shared x-face: every slab set is an x-chain and the chains end at the rank boundary
  1 x 1 x 2  5 x 3 x 2  5 x 3 x 4   the shared face is a z-plane: contiguous node lists
  2 x 2 x 2  5 x 3 x 2  10 x 6 x 4  a corner node held by eight ranks, edge nodes by four, 7 peers each; all-pairs like the
                                    two above, so (d, A d) rides on the halo messages and (r, z) goes as accumulator words
  3 x 1 x 1  5 x 2 x 2  15 x 2 x 2  not all-pairs: the all-reduce fallback and ticketed (r, z), decided collectively
  3 x 3 x 1  5 x 2 x 2  15 x 6 x 2  a middle rank with eight neighbours; nine ranks, not all-pairs

laghos::Partition picks the table's rank grid for each of the five global shapes and rank counts, and 2 x 2 x 1 for the
10 x 6 x 2 zones of the problem-7 case (tests/test_rank_cases.py asserts it); the kernel-level tests build their partition
with the oracle and do not depend on it."""
import zlib

import numpy as np

import shape_cases as sc

BLOCK = (13, 5)
RANK_GRIDS = {
    (2, 1): "one shared edge, all-pairs",
    (1, 2): "the shared edge along x: contiguous node lists",
    (2, 2): "a corner node held by four ranks, three peers each, all-pairs",
    (3, 1): "not all-pairs: only the middle rank sees everyone",
    (3, 2): "edge ranks with corner peers, not all-pairs",
    (3, 3): "a middle rank with eight neighbours",
}
# peers per rank (x fastest), counted by hand
PEERS = {(2, 1): [1, 1], (1, 2): [1, 1], (2, 2): [3, 3, 3, 3], (3, 1): [1, 2, 1], (3, 2): [3, 5, 3, 3, 5, 3],
         (3, 3): [3, 5, 3, 5, 8, 5, 3, 5, 3]}
BLOCK_3D, GRID_3D, ORDER_3D = (5, 3, 2), (2, 1, 1), (2, 1)
# rank grid: (block, what it is the smallest case of)
RANK_GRIDS_3D = {
    (2, 1, 1): ((5, 3, 2), "one shared x-face: the x-chains end at the rank boundary; all-pairs"),
    (1, 1, 2): ((5, 3, 2), "the shared face is a z-plane: contiguous node lists; all-pairs"),
    (2, 2, 2): ((5, 3, 2), "a corner node held by eight ranks, edge nodes by four, 7 peers each; all-pairs"),
    (3, 1, 1): ((5, 2, 2), "not all-pairs: the all-reduce fallback and ticketed (r, z)"),
    (3, 3, 1): ((5, 2, 2), "a middle rank with eight neighbours; nine ranks, not all-pairs"),
}
# peers per rank (x fastest), counted by hand; the most ranks that hold one node; every rank sees every other
PEERS_3D = {(2, 1, 1): [1, 1], (1, 1, 2): [1, 1], (2, 2, 2): [7] * 8, (3, 1, 1): [1, 2, 1], (3, 3, 1): [3, 5, 3, 5, 8, 5, 3, 5, 3]}
HELD_MAX_3D = {(2, 1, 1): 2, (1, 1, 2): 2, (2, 2, 2): 8, (3, 1, 1): 2, (3, 3, 1): 4}
ALL_PAIRS_3D = {(2, 1, 1): True, (1, 1, 2): True, (2, 2, 2): True, (3, 1, 1): False, (3, 3, 1): False}
MESHES = sc.MESHES


def grid_id(pgrid):
    return "x".join(str(n) for n in pgrid) + "ranks"


def n_ranks(pgrid):
    return int(np.prod(pgrid))


def block_of(pgrid):
    """the block of zones every rank of the grid holds: the 2D block, or the 3D table's (a 3D grid outside it: BLOCK_3D)"""
    pgrid = tuple(pgrid)
    return BLOCK if len(pgrid) == 2 else RANK_GRIDS_3D.get(pgrid, (BLOCK_3D,))[0]


def global_shape(pgrid, block=None):
    block = block or block_of(pgrid)
    return tuple(int(b * p) for b, p in zip(block, pgrid))


def _min_rel_gap(v):
    v = np.sort(np.asarray(v, dtype=np.float64))
    return float(np.min(np.diff(v) / v[1:]))


def breaks(shape, mesh):
    """per-axis break points of the global `graded` or `equal` mesh of `shape` zones (origin at 0)"""
    assert mesh in MESHES
    if mesh == "equal":
        return sc.breaks(shape, "equal")
    L = sc.AXIS_LENGTHS[:len(shape)]
    seed = zlib.crc32(("shape " + sc.shape_id(shape)).encode())
    for attempt in range(1000):
        rng = np.random.default_rng([seed, attempt])
        w = []
        for a, n in enumerate(shape):
            f = 1.0 + 0.25 * rng.uniform(-1.0, 1.0, n)
            w.append(L[a] * f / f.sum())
        vol = np.ones(1)
        for wa in w:
            vol = np.multiply.outer(vol, wa).reshape(-1)
        if (_min_rel_gap(vol) > 1e-6 and all(np.all(np.abs(np.diff(wa)) > 2e-3 * wa[1:]) for wa in w)
                and all(np.all(np.abs(w[a] * n / L[a] - 1.0) <= 0.29) for a, n in enumerate(shape))):
            break
    else:
        raise AssertionError("no graded mesh with distinct zone volumes found")
    out = []
    for a, n in enumerate(shape):
        b = np.concatenate([[0.0], np.cumsum(w[a])])
        b[-1] = L[a]
        out.append(b)
    return out


def check_graded(prob):
    """the distinct-volume property of a graded mesh, on the (global or rank) problem itself"""
    assert _min_rel_gap(prob.elem_volumes()) > 0.5e-6
    ei = prob.elem_index()
    h = np.stack([np.diff(prob.breaks[a])[ei[:, a]] for a in range(prob.dim)], axis=1)
    for a in range(prob.dim):
        wa = np.diff(prob.breaks[a])
        assert np.all(np.abs(np.diff(wa)) > 1e-3 * wa[1:])
        for b in range(a + 1, prob.dim):
            assert np.all(np.abs(h[:, a] - h[:, b]) > 1e-3 * h[:, a])


_problems = {}


def problems(pgrid, mesh, order, problem=1):
    """(global problem, [rank problems]) of a rank grid - built once, shared, never modified"""
    key = (tuple(pgrid), mesh, tuple(order), problem)
    if key not in _problems:
        from oracle.fem import Problem
        shape = global_shape(pgrid)
        kw = dict(breaks=breaks(shape, mesh), order_v=order[0], order_e=order[1], problem=problem)
        glob = Problem(**kw)
        assert tuple(glob.ne) == shape
        ranks = [Problem(rank=r, pgrid=list(pgrid), **kw) for r in range(n_ranks(pgrid))]
        block = tuple(s // p for s, p in zip(shape, pgrid))
        assert all(tuple(p.ne) == block for p in ranks)
        if mesh == "graded":
            check_graded(glob)
        _problems[key] = (glob, ranks)
    return _problems[key]


def permuted_rank(prob_r, seed):
    """A rank problem under a random renumbering of its nodes and zones (helpers.PermutedProblem), with the neighbour lists
    translated by node_perm - PermutedProblem.__getattr__ would hand through the lists of the base numbering, which name
    other nodes there.  The order within a list stays the base problem's, so both sides still list the same global nodes
    in the same order.  unpermute_nodes / unpermute_zones take a result back to the generator's numbering."""
    from helpers import PermutedProblem

    class PermutedRank(PermutedProblem):
        def neighbors(self):
            nr, lists = self.base.neighbors()
            return nr, [self.node_perm[np.asarray(l, dtype=np.int64)].astype(np.int32) for l in lists]

    return PermutedRank(prob_r, seed=seed)


def unpermute_nodes(perm, v, ncomp=1):
    return np.ascontiguousarray(np.asarray(v).reshape(ncomp, perm.base.N)[:, perm.node_perm]).reshape(-1)


def unpermute_zones(perm, a, per_zone):
    out = np.empty((perm.base.NE, per_zone))
    out[perm.elem_perm] = np.asarray(a).reshape(perm.base.NE, per_zone)
    return out.reshape(-1)


# ---- a rank's zones and nodes in the global numbering, from the integer block offsets ---------------------------------------
def _lex(idx, extent):
    """global lexicographic index (x fastest) of the tensor grid idx[0] x idx[1] (x idx[2]), flattened x fastest"""
    g = np.asarray(idx[0], dtype=np.int64)
    stride = int(extent[0])
    for a in range(1, len(idx)):
        g = (g[None, :] + stride * np.asarray(idx[a], dtype=np.int64)[:, None]).reshape(-1)
        stride *= int(extent[a])
    return g


def node_map(prob_r):
    """global node of every local node of the rank problem"""
    p = prob_r.order_v
    return _lex([prob_r.eoff[a] * p + np.arange(prob_r.nn[a]) for a in range(prob_r.dim)], prob_r.gnn)


def zone_map(prob_r):
    """global zone of every local zone"""
    return _lex([prob_r.eoff[a] + np.arange(prob_r.ne[a]) for a in range(prob_r.dim)], prob_r.global_ne)


def slice_nodes(prob_r, vg, ncomp=1):
    """the rank's piece of a global node vector of ncomp components (byNODES)"""
    m = node_map(prob_r)
    return np.ascontiguousarray(np.asarray(vg).reshape(ncomp, prob_r.global_N)[:, m]).reshape(-1)


def slice_zones(prob_r, ag, per_zone):
    """the rank's piece of a global zone array with per_zone entries per zone (an L2 vector: NL; a quadrature array whose
    zone index is the slowest: NQ * dim^2)"""
    z = zone_map(prob_r)
    return np.ascontiguousarray(np.asarray(ag).reshape(prob_r.global_NE, per_zone)[z]).reshape(-1)


def slice_stress(prob_r, sJg):
    """the rank's piece of a global stressJinvT: dim^2 planes of NE * NQ entries (include/laghos_hip.h)"""
    d2 = prob_r.dim ** 2
    z = zone_map(prob_r)
    return np.ascontiguousarray(np.asarray(sJg).reshape(d2, prob_r.global_NE, prob_r.NQ)[:, z]).reshape(-1)


def slice_state(prob_r, Sg):
    """the rank's piece of a global state [x | v | e]"""
    gH1V = prob_r.dim * prob_r.global_N
    return np.concatenate([slice_nodes(prob_r, Sg[:gH1V], prob_r.dim), slice_nodes(prob_r, Sg[gH1V:2 * gH1V], prob_r.dim),
                           slice_zones(prob_r, Sg[2 * gH1V:], prob_r.NL)])


def gather_nodes(probs, pieces, ncomp=1):
    """The global node vector from the ranks' pieces; every copy of a shared node must hold the same BITS ("shared copies
    identical") - asserted here."""
    gN = probs[0].global_N
    out = np.zeros((ncomp, gN))
    seen = np.zeros(gN, dtype=bool)
    for p, v in zip(probs, pieces):
        m = node_map(p)
        v = np.asarray(v, dtype=np.float64).reshape(ncomp, p.N)
        s = seen[m]
        a, b = out[:, m[s]].view(np.int64), np.ascontiguousarray(v[:, s]).view(np.int64)
        assert np.array_equal(a, b), f"rank {p.rank}: {int(np.sum(a != b))} shared entries differ from a lower rank's copy"
        out[:, m] = v
        seen[m] = True
    assert seen.all()
    return out.reshape(-1)


def gather_zones(probs, pieces, per_zone):
    out = np.zeros((probs[0].global_NE, per_zone))
    for p, v in zip(probs, pieces):
        out[zone_map(p)] = np.asarray(v).reshape(p.NE, per_zone)
    return out.reshape(-1)
