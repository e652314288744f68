"""The file logic of the driver's `-hist` time history (laghos_amd/host/history.cpp through host_lib, no GPU): the header,
row formatting that reads back exactly, trimming on restart, and write failures that are reported."""
import os
import struct

import numpy as np
import pytest

from laghos_amd import host_lib

HEADER = ("# cycle t dt rk_steps repeats mass volume ie ke total d_total px py pz detj_min detj_min_rank detj_min_zone rho_min rho_max "
          "e_min e_max p_max v_max n_inverted n_negative_e n_nonfinite")
INT_COLS = ("cycle", "rk_steps", "repeats", "detj_min_rank", "detj_min_zone", "n_inverted", "n_negative_e", "n_nonfinite")


def bits(x):
    return struct.pack("<d", x)


def diag(**kw):
    """the 20 doubles of lgh_diagnostics with some of them set by name"""
    from laghos_amd.context import DIAG_NAMES
    d = np.arange(1.0, 21.0) * 0.1
    d[14:19] = [3, 4, 5, 6, 1]
    d[19] = 0.0
    for k, v in kw.items():
        d[DIAG_NAMES.index(k)] = v
    return d


def parse(row):
    assert row.endswith("\n") and row.count("\n") == 1
    cells = row[:-1].split(" ")
    assert len(cells) == len(host_lib.HISTORY_COLUMNS)
    return dict(zip(host_lib.HISTORY_COLUMNS, cells))


def test_header():
    assert host_lib.host_history_header() == HEADER
    assert tuple(HEADER[2:].split(" ")) == host_lib.HISTORY_COLUMNS


def test_rows_read_back_exactly():
    awkward = [0.1, 1.0 / 3.0, np.nextafter(1.0, 2.0), 5e-324, 1.7976931348623157e308, -2.2250738585072014e-308, 123456789.123456789,
               -0.0, 0.0, np.inf, -np.inf]
    for i, x in enumerate(awkward):
        d = diag(mass=x, e_min=-x, p_max=x, detj_min=x)
        r = parse(host_lib.host_history_row(7 + i, x, -x, 30, 2, d, 0.25))
        for k, want in (("t", x), ("dt", -x), ("mass", x), ("e_min", -x), ("p_max", x), ("detj_min", x)):
            assert bits(float(r[k])) == bits(want), (k, x, r[k])
        assert r["cycle"] == str(7 + i) and r["rk_steps"] == "30" and r["repeats"] == "2"
        assert bits(float(r["total"])) == bits(d[2] + d[3]) and bits(float(r["d_total"])) == bits(d[2] + d[3] - 0.25)
    r = parse(host_lib.host_history_row(1, 0.5, 0.25, 1, 0, diag(ie=np.nan, e_max=-np.nan), 1.0))
    assert r["ie"] == r["e_max"] == r["total"] == r["d_total"] == "nan" and np.isnan(float(r["ie"]))
    # integers are printed as integers, also the large ones; the zone and its rank come in the header's order
    r = parse(host_lib.host_history_row(123456, 1.0, 1.0, 2 ** 31 + 5, 0, diag(n_inverted=7077888.0, detj_min_zone=32767.0, detj_min_rank=3.0), 0.0))
    assert r["rk_steps"] == str(2 ** 31 + 5) and r["n_inverted"] == "7077888" and r["detj_min_zone"] == "32767" and r["detj_min_rank"] == "3"
    for k in INT_COLS:
        assert r[k].lstrip("-").isdigit(), k
    # equal bits, equal bytes
    assert host_lib.host_history_row(3, 0.1, 0.2, 4, 1, diag(), 0.3) == host_lib.host_history_row(3, 0.1, 0.2, 4, 1, diag(), 0.3)


def rows_for(cycles):
    return "".join(host_lib.host_history_row(c, 0.01 * c, 0.01, 4 * c, 0, diag(mass=1.0 + c), 0.5) for c in cycles)


def test_start_append_and_trim(tmp_path):
    path = str(tmp_path / "deep" / "er" / "run_history.csv")        # the directory chain is created
    rows = rows_for([0, 2, 4, 6])
    assert host_lib.host_history_write(path, rows) == 4
    whole = HEADER + "\n" + rows
    assert open(path).read() == whole
    lines = whole.splitlines(keepends=True)
    # at a cycle that is present: it stays, the later ones go
    assert host_lib.host_history_write(path, keep_upto=4) == 3
    assert open(path).read() == "".join(lines[:4])
    # at a cycle that is absent (odd): nothing more goes; and the run appends
    assert host_lib.host_history_write(path, rows_for([6]), keep_upto=3) == 3
    assert open(path).read() == "".join(lines[:3]) + lines[4]
    # beyond the end: nothing is dropped
    before = open(path).read()
    assert host_lib.host_history_write(path, keep_upto=100) == 3
    assert open(path).read() == before
    # starting anew replaces the file
    assert host_lib.host_history_write(path) == 0
    assert open(path).read() == HEADER + "\n"
    assert not os.path.exists(path + ".tmp")


def test_trim_drops_a_partial_last_line(tmp_path):
    path = str(tmp_path / "run_history.csv")
    rows = rows_for([0, 1, 2])
    with open(path, "w") as f:
        f.write(HEADER + "\n" + rows + rows_for([3])[:37])          # a killed run: the row of cycle 3 is incomplete
    assert host_lib.host_history_write(path, rows_for([4]), keep_upto=3) == 4
    assert open(path).read() == HEADER + "\n" + rows + rows_for([4])
    # a partial line whose cycle is complete and small enough is dropped all the same
    with open(path, "w") as f:
        f.write(HEADER + "\n" + rows[:-1])
    assert host_lib.host_history_write(path, keep_upto=10) == 2
    assert open(path).read() == HEADER + "\n" + rows_for([0, 1])


def test_missing_and_foreign_files(tmp_path):
    path = str(tmp_path / "run_history.csv")
    assert host_lib.host_history_write(path, rows_for([5]), keep_upto=4) == 1     # missing: started anew with the header
    assert open(path).read() == HEADER + "\n" + rows_for([5])
    open(path, "w").close()                                                       # empty (killed before the header): the same
    assert host_lib.host_history_write(path, keep_upto=4) == 0
    assert open(path).read() == HEADER + "\n"
    with open(path, "w") as f:
        f.write("something else\n1 2 3\n")
    with pytest.raises(RuntimeError, match="not the header"):
        host_lib.host_history_write(path, keep_upto=4)
    assert open(path).read() == "something else\n1 2 3\n"                         # refused, not touched


def test_unwritable_directory_is_reported(tmp_path):
    blocker = tmp_path / "file"
    blocker.write_text("x")
    path = str(blocker / "run_history.csv")                                       # its "directory" is a file: nobody can write there
    with pytest.raises(RuntimeError, match="run_history.csv"):
        host_lib.host_history_write(path)
    with pytest.raises(RuntimeError, match="run_history.csv"):
        host_lib.host_history_write(path, rows_for([1]), keep_upto=0)
