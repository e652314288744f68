"""The output bits of the four lattice entries - lgh_sample_fields, lgh_sample_derived, lgh_sample_faces, the gauges - against
tests/golden/lattice_bits.json: one SHA-256 per case, entry and output array.

The file was recorded on an MI355X at the PARENT of the commit that added this test; that commit moved the host side of the
four launches into lgh_sample.hpp and left the kernels' text alone, and this test is what says that no output bit moved.  The
volume kernel, the face kernel and the gauge kernel each hold a sum-factorised contraction of their own and promise each other's
bits at the same point: this is the pin of those bits for whoever changes one of them.  A mismatch is a finding to resolve (an
FMA contracted differently in an epilogue, a reordered sum), not a tolerance to widen.  Where a change of the bits is intended,
re-record on the GPU at the commit whose bits are meant to hold:

    python tests/golden/make_lattice_bits.py

Cases (tests/golden/make_lattice_bits.py builds them and computes the hashes for both sides): the smallest at which these
kernels can go wrong - 1D 257 zones Q3Q2, 2D 3 x 2 Q4Q3, 3D 3 x 2 x 2 Q2Q1 and Q5Q4, 3D 5 x 5 x 3 Q3Q2 (75 zones: a multiple of
no zones-per-workgroup), R1 = 2 (several zones or faces per workgroup), 4, 9 (729 > 256 points per zone: three points per thread in 3D,
R1 > D1D); every output of every entry; shuffled face lists with repeats; 7 gauges with a corner and a face point; and two
emulated ranks, in 2D and in 3D, for the rows of the gauges another rank owns (lgh_gauges_create refuses a gauge that no rank
owns, and tests/rank_cases.py has no 1D rank grid: in 1D no gauge with zone = -1 is hashed, and a 1D gauge kernel meets an
empty gauge only in the unused wavefronts of its last workgroup, which store nothing)."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_lattice_bits", os.path.join(GOLDEN, "make_lattice_bits.py"))
mlb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mlb)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "lattice_bits.json")) as f:
        return json.load(f)["cases"]


def test_the_file_holds_the_cases(recorded):
    assert set(recorded) == set(mlb.CASES) | set(mlb.TWO_RANKS)
    for name, (zones, _, _) in mlb.CASES.items():
        entries = {f"{e}-R{R1}" for R1 in mlb.R1S for e in (("fields", "derived") + (("faces",) if len(zones) > 1 else ()))} | {"gauges"}
        assert set(recorded[name]) == entries, name
        for R1 in mlb.R1S:
            assert set(recorded[name][f"fields-R{R1}"]) == set(mlb.FIELDS)
            assert set(recorded[name][f"derived-R{R1}"]) == set(mlb.DERIVED) - ({"vorticity"} if len(zones) == 1 else set())
            if len(zones) > 1:
                assert set(recorded[name][f"faces-R{R1}"]) == set(mlb.FACES)
        assert set(recorded[name]["gauges"]) == {"mass", "rows"}
    for name in mlb.TWO_RANKS:
        assert set(recorded[name]) == {"gauges-rank0", "gauges-rank1"}


@pytest.mark.parametrize("name", list(mlb.CASES) + list(mlb.TWO_RANKS))
def test_the_bits_are_the_recorded_ones(recorded, name):
    got = mlb.hashes(name)
    differ = [(entry, k) for entry, arrays in recorded[name].items() for k, h in arrays.items() if got.get(entry, {}).get(k) != h]
    print(f"{name}: {sum(len(a) for a in got.values())} arrays, {len(differ)} differ")
    assert not differ, (name, differ)
    assert set(got) == set(recorded[name])
