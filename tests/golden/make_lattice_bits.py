"""Emit tests/golden/lattice_bits.json: SHA-256 of every output array of the four lattice entries - lgh_sample_fields,
lgh_sample_derived, lgh_sample_faces and the gauges - on small seeded cases.  tests/test_gpu_lattice_bits.py recomputes the
hashes with hashes() below and compares: a change of these kernels that moves one bit of one output shows.

Needs a GPU and the built library.  The cases are those of tests/test_gpu_sample.py (its Case: curved mesh, random v, e with
negative values, random density dofs, a gamma per zone) on the meshes and orders of CASES, R1 of R1S:

  fields, derived   every output (the vorticity not in 1D)
  faces (2D, 3D)    every (zone, face) of the mesh in a seeded shuffled order, the first three again at the end: the count is no
                    multiple of the faces per workgroup and the normal axes mix inside a workgroup; all eleven outputs
  gauges            7 gauges (no multiple of the 4 per workgroup): one at a corner (xi = 0), one on a face (one coordinate
                    exactly 1), five seeded interior points; gauges_mass and one drained sample
  2 ranks           lgh_gauges_create refuses a set in which no rank owns a gauge, so the row of a gauge with zone = -1 exists
                    on several ranks only: the 2D problem of tests/test_gpu_gauges.py::test_two_ranks_drain_the_rows_of_one and
                    the 3D one of tests/rank_cases.py on two emulated ranks each, 7 gauges, each rank's masses (-0.0 where the
                    other rank owns the gauge) and drained rows (tests/rank_cases.py has no 1D rank grid)

    python tests/golden/make_lattice_bits.py [output file]
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

CASES = {"1D-257-Q3Q2": ((257,), 3, 2), "2D-3x2-Q4Q3": ((3, 2), 4, 3), "3D-3x2x2-Q2Q1": ((3, 2, 2), 2, 1),
         "3D-3x2x2-Q5Q4": ((3, 2, 2), 5, 4), "3D-5x5x3-Q3Q2": ((5, 5, 3), 3, 2)}
R1S = (2, 4, 9)
FIELDS = ("x", "v", "e", "rho", "p")
DERIVED = ("detj", "grad_v", "div_v", "vorticity", "sound_speed")
FACES = FIELDS + DERIVED + ("area_normal",)
TWO_RANKS = {"2D-2ranks-Q3Q2": ((2, 1), (3, 2)), "3D-2ranks-Q2Q1": ((2, 1, 1), (2, 1))}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<f8").tobytes()).hexdigest()


def ncomp(k, dim):
    return {"x": dim, "v": dim, "grad_v": dim * dim, "vorticity": 3 if dim == 3 else 1, "area_normal": dim}.get(k, 1)


def run(c, call, names, npts):
    """the hashes of the outputs `names` of one entry; NaN-filled before the call: an entry left unwritten shows"""
    out = {k: c.ctx.to_dev(np.full(ncomp(k, c.dim) * npts, np.nan)) for k in names}
    call(out)
    c.ctx.sync()
    return {k: sha(t.cpu().numpy()) for k, t in out.items()}


def face_list(c):
    every = np.stack([np.repeat(np.arange(c.NE), 2 * c.dim), np.tile(np.arange(2 * c.dim), c.NE)], 1).astype(np.int32)
    every = every[np.random.default_rng(31 * c.NE + c.dim).permutation(len(every))]
    return np.ascontiguousarray(np.concatenate([every, every[:3]]))


def gauge_points(dim, NE, zones=None):
    """7 gauges: zone (int32) and xi (7, dim)"""
    rng = np.random.default_rng(17 * dim + NE)
    zone = rng.integers(0, NE, 7).astype(np.int32) if zones is None else np.asarray(zones, dtype=np.int32)
    xi = rng.uniform(0.05, 0.95, (7, dim))
    xi[1] = 0.0
    xi[2, dim - 1] = 1.0
    return zone, xi


def case_hashes(name):
    import gauges_ref as gr
    from derived_ref import lattice_tables3
    from test_gpu_gauges import set_up
    from test_gpu_sample import Case
    zones, ok, ot = CASES[name]
    c = Case(zones, ok, ot)
    try:
        dim, res = c.dim, {}
        for R1 in R1S:
            Bh, Gh, Bl = lattice_tables3(ok, ot, R1 - 1)
            NP = c.NE * R1 ** dim
            res[f"fields-R{R1}"] = run(c, lambda o: c.ctx.sample_fields(c.Sd, c.rhod, Bh, Bl, **o), FIELDS, NP)
            names = tuple(k for k in DERIVED if dim > 1 or k != "vorticity")
            res[f"derived-R{R1}"] = run(c, lambda o: c.ctx.sample_derived(c.Sd, Bh, Gh, Bl, **o), names, NP)
            if dim > 1:
                faces = face_list(c)
                res[f"faces-R{R1}"] = run(c, lambda o: c.ctx.sample_faces(c.Sd, c.rhod, Bh, Gh, Bl, faces, **o), FACES, len(faces) * R1 ** (dim - 1))
        set_up(c)
        zone, xi = gauge_points(dim, c.NE)
        h = c.ctx.gauges_create(zone, *gr.tables_at(ok, ot, xi), c.x0d, c.rhod, 1)
        try:
            c.ctx.gauges_sample(h, c.Sd)
            rows = c.ctx.gauges_drain(h)
            res["gauges"] = {"mass": sha(c.ctx.gauges_mass(h)), "rows": sha(rows)}
        finally:
            c.ctx.gauges_destroy(h)
        return res
    finally:
        c.close()


def two_rank_hashes(pgrid, order):
    import rank_cases as rc
    from helpers import deformed_state
    from rank_threads import Ranks
    glob, probs = rc.problems(pgrid, "equal", order)
    S = deformed_state(glob, seed=11, amp=0.05)
    S[2 * glob.H1V::3] *= -1.0                                       # e with negative values
    rng = np.random.default_rng(23)
    zone_g, xi = gauge_points(glob.dim, glob.NE, zones=rng.integers(0, glob.NE, 7))
    zones = []
    for p in probs:
        local = {int(gz): j for j, gz in enumerate(rc.zone_map(p))}
        zones.append(np.array([local.get(int(z), -1) for z in zone_g], dtype=np.int32))
    zones[0][0], zones[1][0] = -1, max(zones[1][0], 0)               # (gauge 0: rank 0 does not own it, whatever the draw)
    zones[1][3], zones[0][3] = -1, max(zones[0][3], 0)               # (gauge 3: rank 1 does not)
    ranks = Ranks(probs, cg_tol=1e-12)
    try:
        def leg(r, op, p):
            h = op.gauges(zones[r], xi, capacity=1)
            op.ctx.gauges_sample(h, op.ctx.to_dev(rc.slice_state(p, S)))
            mass = op.ctx.gauges_mass(h)
            return {"mass": sha(mass), "rows": sha(op.ctx.gauges_drain(h))}, mass
        got = ranks.run(leg)
    finally:
        ranks.close()
    for r in range(2):   # the rows of zone -1 are in the hashes
        mine = zones[r] >= 0
        assert mine.any() and not mine.all() and np.all(np.signbit(got[r][1][~mine]) & (got[r][1][~mine] == 0))
    return {f"gauges-rank{r}": got[r][0] for r in range(2)}


def hashes(name):
    return two_rank_hashes(*TWO_RANKS[name]) if name in TWO_RANKS else case_hashes(name)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "lattice_bits.json")
    doc = {"what": "SHA-256 of the raw little-endian float64 bytes of every output array, per case and entry (make_lattice_bits.py)",
           "cases": {name: hashes(name) for name in list(CASES) + list(TWO_RANKS)}}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", sum(len(e) for c in doc["cases"].values() for e in c.values()), "hashes to", out)


if __name__ == "__main__":
    main()
