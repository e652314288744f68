"""Element grids that are not powers of two, shared by tests/test_shape_cases.py (CPU: the conditions the GPU tests rely
on, on the oracle alone) and tests/test_gpu_shapes_operators.py / test_gpu_shapes_solve.py (every kernel on these grids).

Every other kernel-level parity test runs on 4x2x2, 4x4x4, 8x8x8, 32^3 or 64^3 zones (4x4, 8x8, 16x16 in 2D): rows of 4, 8,
32 or 64 zones, NE a multiple of 16, and - problem 1 on equal zones - one mass factor s_e and one Jac0inv for all zones.
The kernels group zones by constants such grids never stress.  Read off the dispatch code (not the comments):

  slab K1           sets of ES = 5 consecutive zones      lgh_vcg_slab.hip (ES), lgh_vcg_tables.hip::slab_merge_layout
  plane K1          NEB = 256 / (3 Q) zones, one less at Q = 6: 42 (Q1Q0), 21 (Q2Q1), 13 (Q3Q2)
                                                          lgh_vcg_k1.hip::launch_vcg_plane
  plane K1, D >= 5  5 zones (Q4Q3), 4 zones (Q5Q4), also with two lanes per plane
                                                          lgh_vcg_k1.hip::vcg_resolve_k1 (launch_vcg_plane_ho<5, 8, HY, 5>, <6, 10, 2, 4>)
  column K1         256 / Q^2 zones: 64, 16, 7, 4, 2 for Q1Q0 ... Q5Q4
                                                          lgh_vcg_k1.hip::launch_vcg_apply
  Kronecker K1      64, 32, 16 zones at D1D = 2, 3, 4; 3 (LGH_KRON_NEB=0: 8) at D1D = 5; 2 (4) at D1D = 6
                                                          lgh_vcg_k1.hip::vcg_resolve_k1
  L2 Kronecker      256, 128, 64, 32 zones at L1D = 1 ... 4; 10 (LGH_L2_NEB=0: 16) at L1D = 5
                                                          lgh_mass.hip::launch_l2_kron
  mass column forms, force kernels, 2D point form of the quadrature update
                    256 / Q^2 zones                       lgh_common.hpp::zones_per_wg
  K2                node ranges over max(4 CUs, N / 1024 rounded up to 8) workgroups (LGH_K2_GRID=<n>: n per CU), every
                    second launch with the update of x        lgh_vcg.hip (grid2), vcg_launch_k2p

NE of the shapes below: 1, 4, 5, 6, 5, 5, 42, 30, 22, 26, 14, 17, 27 - 1 is ragged against everything; 17 is prime and
ragged against every group size up to 16; 42 = 2 * 3 * 7 is ragged against 4, 5, 8, 10, 13, 16, 32, 64; none is a
multiple of 16; the 2D grids have 1, 5, 5, 21, 26, 17 zones against point-form batches of 64, 16, 7, 4 (Q = 2, 4, 6, 8).

Two meshes per shape, both oracle.fem.Problem(breaks=...):
  graded  every axis its own length (1.0, 1.25, 1.5), zone widths from a fixed seed within +-30 % of the axis mean: every
          zone has its own volume - hence its own s_e - and hx != hy != hz everywhere (a kernel that reads a neighbour's
          factor, or swaps y and z in a per-zone quantity, is wrong by per cent);
  equal   the same lengths, equal widths along each axis (hx != hy != hz still; one s_e) - what the C++ driver's
          -nx/-ny/-nz -Sx/-Sy/-Sz builds, break for break."""
import zlib

import numpy as np

AXIS_LENGTHS = (1.0, 1.25, 1.5)
ES = 5  # zones of a set of the slab K1

# (nx, ny, nz): what the shape is the smallest case of / which grouping it is ragged against
SHAPES_3D = {
    (1, 1, 1): "one zone: every grouping is ragged (5, 13, 7, 16, 64, ...); K2 on 64 nodes, all but one workgroup without a node",
    (4, 1, 1): "fewer zones than one slab set (5); one ragged column batch (7 at Q3Q2)",
    (5, 1, 1): "exactly one chain set, no ragged set",
    (6, 1, 1): "a chain set followed by a one-zone set that shares a face with it",
    (1, 5, 1): "five consecutive zones that are y-neighbours: a full set that must not merge",
    (1, 1, 5): "five consecutive zones that are z-neighbours: a full set that must not merge",
    (7, 3, 2): "42 zones, 5 and 7 coprime: sets start at every offset of a row and straddle rows; ragged against 4, 5, 8, 10, 13, 16",
    (10, 3, 1): "30 zones, every set is a chain; ragged against 4, 7, 8, 13, 16",
    (11, 2, 1): "22 zones: two chains, a straddling set, a chain at offset 4, a ragged pair; ragged against 3, 4, 5, 7, 8, 10, 13, 16",
    (13, 1, 2): "26 zones: exactly two plane batches of 13; ragged against 3, 4, 5, 7, 8, 10, 16",
    (14, 1, 1): "14 zones: a plane batch of 13 and one zone; exactly two column batches of 7",
    (17, 1, 1): "17 zones, prime: ragged against every group size from 2 to 16",
    (3, 3, 3): "27 zones in rows of 3: no chain anywhere; ragged against 2, 4, 5, 7, 8, 10, 13, 16",
}
# orders other than Q3Q2 run on these four (Q1Q0, Q2Q1, Q4Q3, Q5Q4)
SHAPES_3D_ALL_ORDERS = [(1, 1, 1), (7, 3, 2), (11, 2, 1), (17, 1, 1)]
SHAPES_2D = {
    (1, 1): "one zone",
    (5, 1): "5 zones in a row; ragged against 4, 7, 16, 64",
    (1, 5): "5 zones in a column",
    (7, 3): "21 zones; ragged against 4, 16, 64 (three full batches of 7 at Q3Q2)",
    (13, 2): "26 zones; ragged against 4, 7, 16, 64",
    (17, 1): "17 zones, prime",
}
ORDERS_3D_OTHER = [(1, 0), (2, 1), (4, 3), (5, 4)]
ORDERS_2D = [(1, 0), (2, 1), (3, 2), (4, 3)]
MESHES = ("graded", "equal")


def shape_id(shape):
    return "x".join(str(n) for n in shape)


def order_id(order):
    return f"Q{order[0]}Q{order[1]}"


def cases_3d():
    """[(shape, order)]: Q3Q2 on every 3D shape, the other orders on SHAPES_3D_ALL_ORDERS"""
    return [(s, (3, 2)) for s in SHAPES_3D] + [(s, o) for o in ORDERS_3D_OTHER for s in SHAPES_3D_ALL_ORDERS]


def cases_2d():
    return [(s, o) for o in ORDERS_2D for s in SHAPES_2D]


def all_cases():
    return cases_3d() + cases_2d()


def case_id(case):
    return f"{shape_id(case[0])}-{order_id(case[1])}"


def solve_mesh(order):
    """The mesh whole right-hand sides run on (tests/test_shape_cases.py asserts the condition): graded up to Q3Q2; at
    Q4Q3 and Q5Q4 the unpreconditioned Bernstein mass of a graded mesh has as many distinct eigenvalue clusters as zones
    and the energy CG needs 4 000 to 26 000 iterations at 1e-14 - the equal mesh there (at most 150)."""
    return "graded" if order[0] <= 3 else "equal"


CG_TOL, CG_CAP = 1e-14, 4000


def _min_rel_gap(v):
    v = np.sort(np.asarray(v, dtype=np.float64))
    return np.inf if v.size < 2 else float(np.min(np.diff(v) / v[1:]))


def breaks(shape, mesh):
    """per-axis break points of the shape's `graded` or `equal` mesh (origin at 0: the Sedov source sits there)"""
    assert mesh in MESHES
    L = AXIS_LENGTHS[:len(shape)]
    if mesh == "equal":
        return [np.array([L[a] * i / n for i in range(n + 1)]) for a, n in enumerate(shape)]
    # widths mean * (1 + 0.25 u), u uniform in (-1, 1), rescaled to the axis length; the seed is a fixed function of the
    # shape, and the first draw is taken whose widths are still within +-30 % of the mean after the rescaling and whose
    # zone volumes are pairwise distinct by more than 2e-3
    seed = zlib.crc32(("shape " + shape_id(shape)).encode())
    for attempt in range(1000):
        rng = np.random.default_rng([seed, attempt])
        w = []
        for a, n in enumerate(shape):
            f = 1.0 + 0.25 * rng.uniform(-1.0, 1.0, n)
            w.append(L[a] * f / f.sum())
        vol = np.ones(1)
        for wa in w:
            vol = np.multiply.outer(vol, wa).reshape(-1)
        if _min_rel_gap(vol) > 2e-3 and all(np.all(np.abs(w[a] * n / L[a] - 1.0) <= 0.29) for a, n in enumerate(shape)):
            break
    else:
        raise AssertionError("no graded mesh with distinct zone volumes found")
    out = []
    for a, n in enumerate(shape):
        assert np.all(np.abs(w[a] * n / L[a] - 1.0) <= 0.30)
        b = np.concatenate([[0.0], np.cumsum(w[a])])
        b[-1] = L[a]
        out.append(b)
    return out


def make_problem(shape, mesh, order, problem=1):
    from oracle.fem import Problem
    prob = Problem(breaks=breaks(shape, mesh), order_v=order[0], order_e=order[1], problem=problem)
    assert tuple(prob.ne) == tuple(shape)
    if mesh == "graded":
        # every zone its own volume (its own s_e); every zone's widths differ between the axes
        assert _min_rel_gap(prob.elem_volumes()) > 1e-3
        ei = prob.elem_index()
        h = np.stack([np.diff(prob.breaks[a])[ei[:, a]] for a in range(prob.dim)], axis=1)
        for a in range(prob.dim):
            for b in range(a + 1, prob.dim):
                assert np.all(np.abs(h[:, a] - h[:, b]) > 1e-3 * h[:, a])
    return prob


def box_volume(shape):
    return float(np.prod(AXIS_LENGTHS[:len(shape)]))


def n_chains(shape):
    """Sets of the slab K1 that are x-chains, from the shape alone: set s holds zones 5 s ... 5 s + 4 (x fastest); it is a
    chain when it is complete and lies inside one row of nx zones."""
    nx, NE = shape[0], int(np.prod(shape))
    return sum(1 for s in range(NE // ES) if nx >= ES and (ES * s) % nx <= nx - ES)


def n_merged(shape):
    """E-vector entries the merged layout sums into the zone to their left: 4 faces of 16 nodes per chain"""
    return 64 * n_chains(shape)


# (counted by hand on the shapes in their order above)
assert [n_chains(s) for s in SHAPES_3D] == [0, 0, 1, 1, 0, 0, 4, 6, 3, 4, 2, 3, 0]
