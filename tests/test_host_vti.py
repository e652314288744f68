"""The writer of the `-map` files (laghos_amd/host/map_output.cpp through host_lib.host_write_vti) against the reader of
tests/vti_reader.py, without a GPU: header, extents, origin and spacing in 1D, 2D and 3D, the order and the bits of the arrays,
the FieldData, and equal bytes for equal input."""
import os

import numpy as np
import pytest

from vti_reader import read_vti

CELL_ORDER = ["n", "vol", "mass", "ie", "ke", "momentum", "pv", "rho_min", "rho_max", "density", "specific_internal_energy", "velocity",
              "pressure"]
GRIDS = {1: ((5,), (-0.5,), (2.0,)), 2: ((4, 3), (0.0, 0.25), (1.0, 1.0)), 3: ((3, 2, 4), (0.1, -1.0, 0.0), (0.7, 1.0, 1e-3))}


def make_rows(dim, cells, seed):
    """rows as lgh_map returns them: counts, sums (momentum above dim exactly 0), extremes; one empty cell and an empty `outside`"""
    rng = np.random.default_rng(seed)
    nc = int(np.prod(cells))
    rows = rng.uniform(0.5, 2.0, (nc + 1, 11))
    rows[:, 0] = rng.integers(1, 50, nc + 1)
    rows[:, 5:8] = rng.uniform(-1, 1, (nc + 1, 3))
    rows[:, 5 + dim:8] = 0.0
    for r in (0, 2):
        rows[r, :9], rows[r, 9], rows[r, 10] = 0.0, np.inf, -np.inf
    rows[3, 4] = np.nan                                   # a poisoned entry travels as it is
    return rows


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_file_layout_and_bits(tmp_path, dim):
    from laghos_amd import host_lib
    cells, lo, hi = GRIDS[dim]
    rows = make_rows(dim, cells, dim)
    nc = int(np.prod(cells))
    path = host_lib.host_write_vti(tmp_path / "a" / "run_map", dim, cells, lo, hi, rows, 17, cycle=12, time=0.3125)
    assert path == os.path.join(str(tmp_path / "a" / "run_map"), "cycle_000012.vti") and os.path.exists(path)
    f = read_vti(path)
    full = list(cells) + [0] * (3 - dim)
    assert f["whole_extent"] == [0, full[0], 0, full[1], 0, full[2]] and f["piece_extent"] == f["whole_extent"]
    assert f["origin"] == list(lo) + [0.0] * (3 - dim)
    assert f["spacing"] == [(hi[c] - lo[c]) / cells[c] for c in range(dim)] + [1.0] * (3 - dim)
    assert f["field_order"] == ["TIME", "CYCLE", "N_EXCLUDED", "OUTSIDE"] and f["cell_order"] == CELL_ORDER
    assert all(f["types"][k] == "Float64" for k in CELL_ORDER + ["TIME", "OUTSIDE"])
    assert f["field"]["TIME"][0] == 0.3125 and f["field"]["CYCLE"][0] == 12 and f["field"]["N_EXCLUDED"][0] == 17
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    assert np.array_equal(bits(f["field"]["OUTSIDE"]), bits(rows[0]))
    grid = rows[1:]
    for k, name in ((0, "n"), (1, "vol"), (2, "mass"), (3, "ie"), (4, "ke"), (8, "pv"), (9, "rho_min"), (10, "rho_max")):
        assert f["cell"][name].shape == (nc,) and np.array_equal(bits(f["cell"][name]), bits(grid[:, k])), name
    assert f["cell"]["momentum"].shape == (nc, 3) and np.array_equal(bits(f["cell"]["momentum"]), bits(grid[:, 5:8]))
    with np.errstate(all="ignore"):
        ratio = lambda a, b: np.where(b != 0, a / b, np.nan)
        want = dict(density=ratio(grid[:, 2], grid[:, 1]), specific_internal_energy=ratio(grid[:, 3], grid[:, 2]), pressure=ratio(grid[:, 8], grid[:, 1]))
        vel = np.stack([ratio(grid[:, 5 + c], grid[:, 2]) if c < dim else np.zeros(nc) for c in range(3)], axis=1)
    for name, w in want.items():
        assert np.array_equal(f["cell"][name], w, equal_nan=True), name
    assert np.array_equal(f["cell"]["velocity"], vel, equal_nan=True)
    # the empty cell: NaN where the divisor is 0, 0 in a velocity component above the dimension; the poisoned entry is there
    assert np.isnan(f["cell"]["density"][1]) and np.isnan(f["cell"]["velocity"][1, :dim]).all() and np.all(f["cell"]["velocity"][1, dim:] == 0.0)
    assert np.isnan(f["cell"]["ke"][2])


def test_equal_input_gives_equal_bytes(tmp_path):
    from laghos_amd import host_lib
    cells, lo, hi = GRIDS[3]
    rows = make_rows(3, cells, 5)
    a = host_lib.host_write_vti(tmp_path / "a", 3, cells, lo, hi, rows, 0, cycle=3, time=0.5)
    b = host_lib.host_write_vti(tmp_path / "b", 3, cells, lo, hi, rows.copy(), 0, cycle=3, time=0.5)
    assert open(a, "rb").read() == open(b, "rb").read()
    other = rows.copy()
    other[4, 3] = np.nextafter(other[4, 3], 2.0)
    c = host_lib.host_write_vti(tmp_path / "c", 3, cells, lo, hi, other, 0, cycle=3, time=0.5)
    assert open(a, "rb").read() != open(c, "rb").read()


def test_an_unwritable_directory_is_an_error(tmp_path):
    from laghos_amd import host_lib
    blocker = tmp_path / "file"
    blocker.write_text("x")
    cells, lo, hi = GRIDS[1]
    with pytest.raises(RuntimeError, match="cannot write"):
        host_lib.host_write_vti(blocker / "sub", 1, cells, lo, hi, make_rows(1, cells, 1), 0, cycle=0, time=0.0)
