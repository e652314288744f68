"""tests/loads_ref.py, the numpy reference of lgh_loads, held to three identities on every shape and order of the GPU tests
(CPU only), within the bound of that file's docstring (the surface row's sum |addend| on one side, the volume sum's on the other):
  xn(surface)   == dim sum w detJ        - the divergence theorem; exact at the default rule (x.N has degree at most 3k - 1
                                           per direction, the rule is exact to 3k + ot - 1);
  flux(surface) == sum w detJ div v;
  uniform e, rho and gamma: |force_c(surface)| <= bound with pa as sum |addend| - a uniform pressure on a closed surface
  exerts no net force.
Beside them: the walls add up to the surface, a listed-twice face counts twice, and a NaN coordinate excludes the points of
the faces that hold the node."""
import numpy as np
import pytest

import loads_ref as lr


@pytest.fixture(scope="module")
def data():
    made = {}

    def get(zones_id, order):
        key = (zones_id, order)
        if key not in made:
            d = lr.case_data(lr.ZONES[zones_id], *order)
            made[key] = (d, lr.FacePoints(d))
        return made[key]
    return get


@pytest.mark.parametrize("zones_id,order", lr.CASES, ids=lr.IDS)
def test_divergence_theorem_and_swept_volume(data, zones_id, order):
    d, fp = data(zones_id, order)
    dim = d["dim"]
    groups = lr.wall_groups(d)
    ref = lr.loads_reference(fp, lr.listing(groups), len(groups))
    assert ref["n_excluded"] == 0 and ref["rows"][0, 0] == len(groups[0][1]) * d["Q"] ** (dim - 1)
    vol, vol_abs, dvol, dvol_abs = lr.volume_integrals(d)
    k = ref["kappa"][0]
    for name, got, want, ab in (("xn", ref["rows"][0, 8], dim * vol, ref["abs"][0, 8] + dim * vol_abs),
                                ("flux", ref["rows"][0, 7], dvol, ref["abs"][0, 7] + dvol_abs)):
        b = lr.bound(dim, d["D"], d["L"], k, ab)
        print(f"{zones_id} Q{order[0]}Q{order[1]} {name}: |diff| / bound {abs(got - want) / b:.4f} (kappa {k:.2f})")
        assert abs(got - want) <= b, (name, got, want, b)
    assert vol > 0 and abs(ref["rows"][0, 8]) > 0.5 * dim * vol
    # the walls add up to the surface
    walls = ref["rows"][1:]
    assert walls[:, 0].sum() == ref["rows"][0, 0] and (walls[:, 0] > 0).all()
    for c in lr.SUM_COLS:
        b = lr.bound(dim, d["D"], d["L"], ref["kappa"].max(), 2 * ref["abs"][0, c])
        assert abs(walls[:, c].sum() - ref["rows"][0, c]) <= b, lr.COLS[c]
    assert ref["rows"][0, 9] == walls[:, 9].min() and ref["rows"][0, 10] == walls[:, 10].max()
    assert np.all(ref["rows"][:, 2 + dim:5].view(np.uint64) == 0)


@pytest.mark.parametrize("zones_id,order", lr.CASES, ids=lr.IDS)
def test_uniform_pressure_exerts_no_net_force(data, zones_id, order):
    d, _ = data(zones_id, order)
    dim, H1V = d["dim"], d["dim"] * d["N"]
    S = d["S"].copy()
    S[2 * H1V:] = 0.75
    fp = lr.FacePoints(d, S=S, rho=np.full(d["rho"].size, 1.5), gamma=np.full(d["NE"], 1.4))
    bf = lr.boundary_faces(d)
    ref = lr.loads_reference(fp, np.concatenate([bf, np.zeros((len(bf), 1), np.int32)], 1), 1)
    row, pa = ref["rows"][0], ref["rows"][0, 5]
    p = 0.4 * 1.5 * 0.75
    assert abs(row[9] - p) <= 1e-13 * p and abs(row[10] - p) <= 1e-13 * p and abs(pa - p * row[1]) <= 1e-12 * pa
    b = lr.bound(dim, d["D"], d["L"], ref["kappa"][0], pa)
    print(f"{zones_id} Q{order[0]}Q{order[1]}: max |force| / bound {np.abs(row[2:2 + dim]).max() / b:.4f}")
    assert np.all(np.abs(row[2:2 + dim]) <= b), (row[2:5], b)


def test_listed_twice_and_a_nan_coordinate(data):
    d, fp = data("3D-3x2x2", (2, 1))
    faces = lr.all_faces(d)
    once = lr.loads_reference(fp, np.concatenate([faces, np.zeros((len(faces), 1), np.int32)], 1), 1)
    twice = lr.loads_reference(fp, np.concatenate([np.concatenate([faces, faces]), np.zeros((2 * len(faces), 1), np.int32)], 1), 1)
    assert twice["rows"][0, 0] == 2 * once["rows"][0, 0] and np.array_equal(twice["rows"][0, 1:9], 2 * once["rows"][0, 1:9])
    # all faces of all zones: every interior face from both sides, with opposite normals - the areas double, x.N cancels inside
    surf = lr.loads_reference(fp, lr.listing(lr.wall_groups(d)[:1]), 1)
    assert abs(once["rows"][0, 8] - surf["rows"][0, 8]) <= lr.bound(3, d["D"], d["L"], once["kappa"][0], once["abs"][0, 8])
    hm = d["h1map"].reshape(d["NE"], -1)
    node = hm[5, 0]
    S = d["S"].copy()
    S[d["N"] + node] = np.nan
    bad = lr.loads_reference(lr.FacePoints(d, S=S), np.concatenate([faces, np.zeros((len(faces), 1), np.int32)], 1), 1)
    from faces_ref import face_nodes
    holders = sum(node in hm[e, face_nodes(3, d["D"], f)] for e, f in faces)
    assert holders >= 3 and bad["n_excluded"] == holders * d["Q"] ** 2
    assert bad["rows"][0, 0] == once["rows"][0, 0] - bad["n_excluded"] and np.isfinite(bad["rows"]).all()
