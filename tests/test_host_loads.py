"""The host side of `-loads` without a GPU: the options and every refusal of the driver (the `laghos` executable, as
tests/test_host_cli.py: exit status 1, the complete stdout and stderr, nothing created under a fresh -k base - every one of them
comes before the first GPU call), the text of the rows (laghos_amd/host/loads_output.cpp through host_lib), and the file on a
restart (the logic of history.cpp over the header of this file)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from laghos_amd import host_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "laghos_amd", "laghos")
HEADER = "cycle t name n area fx fy fz pa p_mean power flux xn p_min p_max"
TO_FA = "Laghos does not support PA in 1D. Switching to FA.\n"
NO_LOADS_1D = "-loads: pressure loads are taken on zone faces in 2D and 3D, this mesh is 1D"
NEEDS_LOADS = "-loads-plane adds rows to the -loads file: it needs -loads"
EIGHT = sum((["-loads-plane", "x", str(k)] for k in range(8)), [])

# (arguments, stderr without `laghos: ` and its newline[, stdout])
REFUSED = [
    (["-loads"], "missing value for -loads"),
    (["--loads-steps"], "missing value for --loads-steps"),
    (["-loads", "0"], "-loads / --loads-steps must be at least 1, got 0"),
    (["--loads-steps", "-2"], "-loads / --loads-steps must be at least 1, got -2"),
    (["-loads", "abc"], "-loads / --loads-steps must be at least 1, got abc"),
    (["-loads-plane"], "missing value for -loads-plane AXIS K"),
    (["-loads", "2", "-loads-plane", "x"], "missing value for -loads-plane AXIS K"),
    (["--loads-plane", "x"], "missing value for --loads-plane AXIS K"),
    (["-loads", "2", "-loads-plane", "w", "1"], "-loads-plane AXIS K: the axis must be x, y or z, got w"),
    (["-loads", "2", "-loads-plane", "x", "-1"], "-loads-plane x K: K must be a node plane 0 <= K <= n of the zone grid, got -1"),
    (["-loads", "2", "-loads-plane", "x", "1.5"], "-loads-plane x K: K must be a node plane 0 <= K <= n of the zone grid, got 1.5"),
    # -loads-plane without -loads
    (["-loads-plane", "x", "1"], NEEDS_LOADS),
    (["--loads-plane", "z", "0", "-hist", "2"], NEEDS_LOADS),
    (["-dim", "1", "-loads-plane", "x", "1"], NEEDS_LOADS),
    # either option in 1D
    (["-dim", "1", "-loads", "2"], NO_LOADS_1D, TO_FA),
    (["-dim", "1", "-q", "-loads", "2", "-loads-plane", "x", "1"], NO_LOADS_1D),
    (["-m", "data/segment01.mesh", "-fa", "--loads-steps", "1"], NO_LOADS_1D),
    # an axis the mesh does not have
    (["-dim", "2", "-loads", "2", "-loads-plane", "z", "1"], "-loads-plane z 1: the mesh has 2 dimensions, there is no z axis"),
    # K out of range (the default mesh: 2 zones per axis, refined twice)
    (["-loads", "2", "-loads-plane", "x", "9"], "-loads-plane x 9: K is out of range, the zone grid has node planes 0..8 along x"),
    (["-dim", "2", "-rs", "1", "-loads", "1", "-loads-plane", "y", "4", "--loads-plane", "y", "5"],
     "-loads-plane y 5: K is out of range, the zone grid has node planes 0..4 along y"),
    # a ninth or repeated plane
    (["-loads", "2"] + EIGHT + ["-loads-plane", "y", "0"], "-loads-plane y 0: at most 8 planes, this is the ninth"),
    (["-loads", "2", "-loads-plane", "x", "3", "--loads-plane", "x", "3"], "-loads-plane x 3 is given twice"),
    # accepted where they stand: the message is that of what follows them
    (["-loads", "3", "-loads", "2", "-loads-plane", "x", "3", "-loads-plane", "y", "3", "-bogus"], "unsupported option: -bogus"),
    (["--loads-steps", "2"] + EIGHT + ["-pv-slice", "x", "0", "-ckpt", "0"], "-ckpt / --checkpoint-steps must be at least 1, got 0"),
    (["-loads", "2", "-loads-plane", "x", "8", "-loads-plane", "z", "0", "-fa"], "only the partial-assembly path (-pa) is implemented"),
    (["-pv-slice", "x", "3", "-loads", "1", "-loads-plane", "x", "3", "-fa"], "only the partial-assembly path (-pa) is implemented"),   # slices and planes are apart
]


@pytest.mark.parametrize("case", REFUSED, ids=lambda c: " ".join(c[0]))
def test_the_driver_refuses(case, tmp_path):
    args, message = case[0], case[1]
    stdout = case[2] if len(case) > 2 else ""
    base = tmp_path / "base"
    base.mkdir()
    env = {k: v for k, v in os.environ.items() if k != "LGH_FORCE_MULTI"}
    p = subprocess.run([EXE, "-k", str(base / "out" / "run")] + args, capture_output=True, text=True, timeout=60, cwd=ROOT, env=env)
    assert (p.returncode, p.stdout, p.stderr) == (1, stdout, "laghos: " + message + "\n")
    assert os.listdir(base) == []


def bits(x):
    return struct.pack("<d", x)


def table(n, seed=1):
    rows = np.random.default_rng(seed).uniform(-2.0, 2.0, (n, 11))
    rows[:, 0] = np.arange(1, n + 1) * 16
    rows[:, 1] = np.abs(rows[:, 1]) + 0.1
    return rows


def parse(text):
    out = []
    for line in text.splitlines(keepends=True):
        assert line.endswith("\n")
        cells = line[:-1].split(" ")
        assert len(cells) == len(host_lib.LOADS_FILE_COLUMNS)
        out.append(dict(zip(host_lib.LOADS_FILE_COLUMNS, cells)))
    return out


def test_header():
    assert host_lib.host_loads_header() == HEADER and tuple(HEADER.split(" ")) == host_lib.LOADS_FILE_COLUMNS


def test_rows_read_back_exactly():
    names = ["surface", "x0", "x1", "y0", "y1", "plane_y2"]
    awkward = [0.1, 1.0 / 3.0, np.nextafter(1.0, 2.0), 5e-324, 1.7976931348623157e308, -2.2250738585072014e-308, 123456789.123456789, -0.0, 0.0]
    for i, x in enumerate(awkward):
        rows = table(len(names), seed=i)
        rows[2, 1:] = x
        rows[3, [2, 6, 9]] = -x
        text = host_lib.host_loads_text(40 + i, x, names, rows)
        got = parse(text)
        assert [g["name"] for g in got] == names and all(g["cycle"] == str(40 + i) and bits(float(g["t"])) == bits(x) for g in got)
        for r, g in enumerate(got):
            assert g["n"] == str(int(rows[r, 0])) and g["n"].isdigit()
            for k, name in ((1, "area"), (2, "fx"), (3, "fy"), (4, "fz"), (5, "pa"), (6, "power"), (7, "flux"), (8, "xn"), (9, "p_min"), (10, "p_max")):
                assert bits(float(g[name])) == bits(rows[r, k]), (x, r, name, g[name])
            with np.errstate(all="ignore"):
                assert bits(float(g["p_mean"])) == bits(rows[r, 5] / rows[r, 1]) or (np.isnan(rows[r, 5] / rows[r, 1]) and g["p_mean"] == "nan")
        assert text == host_lib.host_loads_text(40 + i, x, names, rows)          # equal bits, equal bytes
    # an empty row, a poisoned entry, extremes without a finite value
    rows = table(3)
    rows[1] = [0, 0, 0, 0, 0, 0, 0, 0, 0, np.inf, -np.inf]
    rows[2, [2, 5]] = np.nan
    rows[2, 3] = -np.nan
    got = parse(host_lib.host_loads_text(7, 0.5, ["surface", "x0", "plane_z12"], rows))
    assert got[1]["n"] == "0" and got[1]["p_mean"] == "nan" and got[1]["p_min"] == "inf" and got[1]["p_max"] == "-inf" and got[1]["area"] == "0"
    assert got[2]["fx"] == got[2]["fy"] == got[2]["pa"] == got[2]["p_mean"] == "nan" and got[2]["name"] == "plane_z12"
    assert bits(float(got[0]["p_mean"])) == bits(rows[0, 5] / rows[0, 1])
    assert host_lib.host_loads_text(3, 0.0, [], np.zeros((0, 11))) == ""


NAMES = ["surface", "x0", "x1", "y0", "y1"]


def lines_for(cycles):
    return "".join(host_lib.host_loads_text(c, 0.01 * c, NAMES, table(len(NAMES), seed=c)) for c in cycles)


def write_cycles(path, cycles, **kw):
    """start or resume, then one append per cycle, as the driver does"""
    n = host_lib.host_loads_write(path, **kw)
    for c in cycles:
        n = host_lib.host_loads_write(path, lines_for([c]), keep_upto=10 ** 9)
    return n


def test_resume_drops_later_cycles_and_a_partial_line(tmp_path):
    path = str(tmp_path / "deep" / "run_loads.csv")                       # the directory chain is created
    write_cycles(path, [0, 2, 4, 6])
    whole = HEADER + "\n" + lines_for([0, 2, 4, 6])
    assert open(path).read() == whole
    # a restart at cycle 3: the lines of cycles 4 and 6 go, and the run appends what it computes again
    host_lib.host_loads_write(path, lines_for([4]), keep_upto=3)
    assert open(path).read() == HEADER + "\n" + lines_for([0, 2, 4])
    # at a cycle that is present: all its lines stay
    host_lib.host_loads_write(path, keep_upto=2)
    assert open(path).read() == HEADER + "\n" + lines_for([0, 2])
    # a killed run: the third line of cycle 4 is incomplete - the complete lines of cycle 4 stay for a restart at 4 ...
    part = lines_for([4])
    cut = part[:len("".join(part.splitlines(keepends=True)[:2])) + 25]
    with open(path, "w") as f:
        f.write(HEADER + "\n" + lines_for([0, 2]) + cut)
    host_lib.host_loads_write(path, keep_upto=4)
    assert open(path).read() == HEADER + "\n" + lines_for([0, 2]) + "".join(part.splitlines(keepends=True)[:2])
    # ... and go with the partial one for a restart at 3, whose run writes cycle 4 again: the file of the uninterrupted run
    with open(path, "w") as f:
        f.write(HEADER + "\n" + lines_for([0, 2]) + cut)
    host_lib.host_loads_write(path, lines_for([4]), keep_upto=3)
    host_lib.host_loads_write(path, lines_for([6]), keep_upto=10 ** 9)
    assert open(path).read() == whole and not os.path.exists(path + ".tmp")


def test_missing_and_foreign_files(tmp_path):
    path = str(tmp_path / "run_loads.csv")
    host_lib.host_loads_write(path, lines_for([5]), keep_upto=4)                  # missing: started anew with the header
    assert open(path).read() == HEADER + "\n" + lines_for([5])
    open(path, "w").close()                                                       # empty: the same
    host_lib.host_loads_write(path, keep_upto=4)
    assert open(path).read() == HEADER + "\n"
    hist = str(tmp_path / "run_history.csv")                                      # the -hist file of the same run is a foreign file
    host_lib.host_history_write(hist)
    for foreign in (open(hist).read() + "1 2 3\n", "something else\n1 2 3\n"):
        with open(path, "w") as f:
            f.write(foreign)
        with pytest.raises(RuntimeError, match="loads .*run_loads.csv: its first line is not the header of a loads file"):
            host_lib.host_loads_write(path, keep_upto=4)
        assert open(path).read() == foreign                                       # refused, not touched
    with open(path, "w") as f:
        f.write(HEADER + "\nsurface 1 2\n")
    with pytest.raises(RuntimeError, match="does not start with a cycle number"):
        host_lib.host_loads_write(path, keep_upto=4)
    blocker = tmp_path / "file"
    blocker.write_text("x")
    with pytest.raises(RuntimeError, match="run_loads.csv"):
        host_lib.host_loads_write(str(blocker / "run_loads.csv"))
