"""`laghos -map N` through host_lib's sim object and the `laghos` executable (the legs of tests/test_gpu_profile_driver.py): which
files are written and what they hold, that the run itself is untouched, that a restarted run writes the files of its segment
byte for byte, and that bad option values are refused before any GPU work.

`-ms N` takes N + 1 steps as the reference's loop does: `-ms 6 -map 2` writes cycles 0, 2, 4, 6 and the last one, 7; the state
of cycle 6 is the final state of the same run with `-ms 5`.  The files are read by tests/vti_reader.py; their arrays are
compared with Sim.map of the same state bit for bit (the same call on the same state)."""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from vti_reader import read_vti

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "laghos_amd", "laghos")

SEDOV_2D = ["-p", 1, "-dim", 2, "-nx", 8, "-ny", 8, "-ok", 2, "-ot", 1, "-ms", 6]
CYCLES = (0, 2, 4, 6, 7)
SUMS = (("n", 0), ("vol", 1), ("mass", 2), ("ie", 3), ("ke", 4), ("pv", 8), ("rho_min", 9), ("rho_max", 10))


def strs(a):
    return [str(x) for x in a]


def run_sim(args, look=None):
    """one leg: a fresh Sim stepped to its end; look(sim) is evaluated on the final state"""
    from laghos_amd import host_lib
    sim = host_lib.Sim(strs(args) + ["-q"])
    try:
        while True:
            rc = sim.step()
            assert rc >= 0, "a step failed"
            if rc == 0:
                break
        sim.sync()
        return dict(t=sim.t, ti=sim.ti, fp=sim.fingerprint(), repeats=sim.repeats, sizes=sim.sizes(), look=look(sim) if look else None,
                    diag=sim.diagnostics())
    finally:
        sim.close()


def files(base):
    return sorted(glob.glob(base + "_map/cycle_*.vti"))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_as_the_call(f, p, dim):
    """the arrays of a file against the dict of Sim.map on the same state"""
    rows = p["rows"]
    assert np.array_equal(bits(f["field"]["OUTSIDE"]), bits(rows[0])) and f["field"]["N_EXCLUDED"][0] == p["n_excluded"]
    for name, k in SUMS:
        assert np.array_equal(bits(f["cell"][name]), bits(rows[1:, k])), name
    assert np.array_equal(bits(f["cell"]["momentum"]), bits(rows[1:, 5:8]))
    nc = rows.shape[0] - 1
    for name, key in (("density", "rho"), ("specific_internal_energy", "e"), ("pressure", "p")):
        assert np.array_equal(f["cell"][name], p[key].reshape(nc), equal_nan=True), name
    assert np.array_equal(f["cell"]["velocity"][:, :dim], p["v"].reshape(nc, dim), equal_nan=True) and np.all(f["cell"]["velocity"][:, dim:] == 0.0)


def test_files_and_their_content(tmp_path):
    base = str(tmp_path / "out" / "run")
    look = lambda sim: sim.map((16, 12), (0.0, 0.0), (1.0, 1.0))
    A = run_sim(SEDOV_2D + ["-map", 2, "-map-cells", 16, 12, "-k", base], look=look)
    assert [os.path.basename(f) for f in files(base)] == ["cycle_%06d.vti" % c for c in CYCLES] and A["ti"] == 7
    assert sorted(os.listdir(base + "_map")) == ["cycle_%06d.vti" % c for c in CYCLES]      # no collection file
    npts = A["sizes"]["global_NE"] * A["sizes"]["NQ"]
    for cyc in CYCLES:
        f = read_vti(base + "_map/cycle_%06d.vti" % cyc)
        # the default box: the extent of the initial mesh, the unit square
        assert f["whole_extent"] == [0, 16, 0, 12, 0, 0] and f["origin"] == [0.0, 0.0, 0.0] and f["spacing"] == [1.0 / 16, 1.0 / 12, 1.0]
        assert f["field"]["CYCLE"][0] == cyc and (f["field"]["TIME"][0] == 0.0) == (cyc == 0) and f["field"]["N_EXCLUDED"][0] == 0
        assert f["cell"]["n"].sum() + f["field"]["OUTSIDE"][0] == npts
    last = read_vti(base + "_map/cycle_000007.vti")
    assert last["field"]["TIME"][0] == A["t"]
    same_as_the_call(last, A["look"], 2)
    B = run_sim(SEDOV_2D + ["-ms", 5, "-k", base + "_b"], look=look)
    assert B["ti"] == 6
    six = read_vti(base + "_map/cycle_000006.vti")
    assert six["field"]["TIME"][0] == B["t"]
    same_as_the_call(six, B["look"], 2)
    assert not files(base + "_b")
    # nothing is lost or invented: the mass of the cells and of `outside` is the -hist mass, to the bound of the row sums of
    # tests/test_gpu_map.py against lgh_diagnostics (NQ + c and NE + c terms, c = dim ND + 8; every addend is positive here)
    sz = A["sizes"]
    c = 2 * 9 + 8
    bound = ((sz["NQ"] + c) + (sz["global_NE"] + c)) * 2.0 ** -52 * A["diag"]["mass"]
    assert abs(last["cell"]["mass"].sum() + last["field"]["OUTSIDE"][2] - A["diag"]["mass"]) <= bound


def test_the_run_is_untouched(tmp_path):
    outs = []
    for extra in ([], ["-map", 2]):
        k = str(tmp_path / ("exe%d" % len(extra)) / "run")
        p = subprocess.run([EXE] + strs(SEDOV_2D + extra + ["-vs", 1, "-fp", "-k", k]), capture_output=True, text=True, timeout=120, cwd=ROOT)
        assert p.returncode == 0, p.stdout + p.stderr
        outs.append((p.stdout, k))
    clock = re.compile(r"^(.*(?: total time| total time \(seconds\)| rate \(.*\))): .*$")
    plain, with_map = ([clock.sub(r"\1:", l) for l in o[0].splitlines()] for o in outs)
    assert any(l.startswith("step ") for l in plain) and len([l for l in plain if l.startswith("State fingerprint:")]) == 1
    assert [l for l in with_map if l.startswith("Maps:")] == [f"Maps: 5 files, {outs[1][1]}_map/cycle_*.vti"]
    assert [l for l in with_map if not l.startswith("Maps:")] == plain          # the fingerprint line among them
    assert len(files(outs[1][1])) == 5
    f = read_vti(files(outs[1][1])[0])
    assert f["whole_extent"] == [0, 64, 0, 64, 0, 0]                              # the default grid: 64 cells per axis of the mesh
    assert not files(outs[0][1]) and not os.path.exists(os.path.dirname(outs[0][1]))   # without -map: no file, no directory


def test_restart_writes_its_segment_byte_for_byte(tmp_path):
    base, base2 = str(tmp_path / "a" / "run"), str(tmp_path / "b" / "run")
    A = run_sim(SEDOV_2D + ["-map", 2, "-map-cells", 10, 7, "-k", base])
    want = {c: open(base + "_map/cycle_%06d.vti" % c, "rb").read() for c in CYCLES}
    opts = SEDOV_2D + ["-map", 2, "-map-cells", 10, 7, "-ckpt", 3, "-ckpt-keep", 0, "-k", base2]
    B = run_sim(opts)
    assert B["fp"] == A["fp"]
    for c in CYCLES:
        assert open(base2 + "_map/cycle_%06d.vti" % c, "rb").read() == want[c], c
        os.remove(base2 + "_map/cycle_%06d.vti" % c)
    # (`-restart latest` would take the checkpoint written after the last step: the one of cycle 3 is named)
    C = run_sim(opts + ["-restart", f"{base2}_restart/cycle_000003.lgr"])
    assert C["fp"] == A["fp"]
    # the files of its own segment and none for the checkpoint's state or before it; the default box as in the first run
    assert [os.path.basename(f) for f in files(base2)] == ["cycle_000004.vti", "cycle_000006.vti", "cycle_000007.vti"]
    for c in (4, 6, 7):
        assert open(base2 + "_map/cycle_%06d.vti" % c, "rb").read() == want[c], c


def test_1d_sod_and_a_3d_leg(tmp_path):
    base = str(tmp_path / "sod")
    A = run_sim(["-p", 2, "-m", "data/segment01.mesh", "-rs", 3, "-ms", 30, "-map", 10, "-map-cells", 16, "-k", base],
                look=lambda sim: sim.map(16, 0.0, 1.0))
    got = [read_vti(f) for f in files(base)]
    cycles = [int(g["field"]["CYCLE"][0]) for g in got]
    assert cycles == sorted(set(range(0, A["ti"] + 1, 10)) | {A["ti"]}) and A["repeats"] > 0   # (repeated steps write no file)
    npts = A["sizes"]["global_NE"] * A["sizes"]["NQ"]
    for g in got:
        assert g["whole_extent"] == [0, 16, 0, 0, 0, 0] and g["origin"] == [0.0, 0.0, 0.0] and g["spacing"] == [1.0 / 16, 1.0, 1.0]
        assert g["cell"]["n"].sum() == npts and g["field"]["N_EXCLUDED"][0] == 0 and g["field"]["OUTSIDE"][0] == 0 and (g["cell"]["n"] > 0).all()
    first, last = got[0]["cell"], got[-1]["cell"]
    assert abs(first["density"][0] - 1.0) < 1e-12 and abs(first["density"][15] - 0.1) < 1e-12       # Sod: rho = 1 | 0.1
    assert np.abs(first["velocity"]).max() == 0.0 and last["velocity"][:, 0].max() > 0.0              # the fluid moves to the right
    same_as_the_call(got[-1], A["look"], 1)
    # 3D, an explicit box that leaves the lowest layer of zones outside
    base3 = str(tmp_path / "cube")
    look = lambda sim: sim.map((4, 2, 3), (0.0, 0.0, 0.25), (1.0, 1.0, 1.0))
    B = run_sim(["-p", 1, "-dim", 3, "-nx", 4, "-ny", 4, "-nz", 4, "-rs", 0, "-ok", 2, "-ot", 1, "-ms", 3, "-map", 2, "-map-cells", 4, 2, 3,
                 "-map-box", 0, 1, 0, 1, 0.25, 1.0, "-k", base3], look=look)
    assert [int(read_vti(f)["field"]["CYCLE"][0]) for f in files(base3)] == [0, 2, 4]
    f = read_vti(files(base3)[-1])
    assert f["whole_extent"] == [0, 4, 0, 2, 0, 3] and f["origin"] == [0.0, 0.0, 0.25] and f["spacing"] == [0.25, 0.5, 0.25]
    npts = B["sizes"]["global_NE"] * B["sizes"]["NQ"]
    assert f["field"]["OUTSIDE"][0] == npts // 4 and np.all(f["cell"]["n"] == npts // 4 * 3 // 24)
    same_as_the_call(f, B["look"], 3)


@pytest.mark.parametrize("bad,word", [(["-map", 0], "-map"), (["-map", 2, "-map-cells", 0, 4], "-map-cells"), (["-map", 2, "-map-cells", 8], "-map-cells"),
                                      (["-map", 2, "-map-cells", 8, 8, 8], "-map-cells"), (["-map", 2, "-map-cells", 2048, 1024], "-map-cells"),
                                      (["-map", 2, "-map-cells"], "-map-cells"), (["-map", 2, "-map-box", 0, 1], "-map-box"),
                                      (["-map", 2, "-map-box", 0, 1, 0], "-map-box"), (["-map", 2, "-map-box", 0, 1, 1, 1], "-map-box"),
                                      (["-map", 2, "-map-box", 0, 1, 0, "inf"], "-map-box"), (["-map", 2, "-map-box", "nan", 1, 0, 1], "-map-box"),
                                      (["-map-cells", 8, 8], "-map"), (["-map-box", 0, 1, 0, 1], "-map")],
                         ids=["map-0", "cells-0", "cells-1-in-2D", "cells-3-in-2D", "cells-above-the-cap", "cells-empty", "box-1-pair-in-2D", "box-odd",
                              "box-1-1", "box-inf", "box-nan", "cells-without-map", "box-without-map"])
def test_bad_values_are_refused(bad, word, tmp_path):
    k = str(tmp_path / "out" / "run")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")     # no device is visible: a refusal cannot have needed one
    p = subprocess.run([EXE] + strs(SEDOV_2D + bad + ["-k", k]), capture_output=True, text=True, timeout=60, cwd=ROOT, env=env)
    assert p.returncode != 0 and word in p.stderr, p.stdout + p.stderr
    assert "Maps:" not in p.stdout and not os.path.exists(os.path.dirname(k))


def test_unwritable_directory_ends_the_run(tmp_path):
    from laghos_amd import host_lib
    blocker = tmp_path / "file"
    blocker.write_text("x")
    with pytest.raises(RuntimeError):
        host_lib.Sim(strs(SEDOV_2D + ["-map", 1, "-k", str(blocker / "run"), "-q"]))
    p = subprocess.run([EXE] + strs(SEDOV_2D + ["-map", 1, "-k", str(blocker / "run")]), capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode != 0 and "-map" in p.stderr and "Maps:" not in p.stdout


def test_triple_point_writes_files_the_reader_parses(tmp_path):
    """the 2D triple point (problem 3) with `-map 20 -map-cells 256 128`: files at cycle 0, after every 20th accepted step and after
    the last one (`-ms` counts the repeated steps of the start too, so the last cycle is the run's own); the mass of the cells and of
    `outside` is the mass of the diagnostics, to the bound of the row sums"""
    base = str(tmp_path / "tp")
    A = run_sim(["-p", 3, "-m", "data/rectangle01_quad.mesh", "-rs", 1, "-ok", 2, "-ot", 1, "-tf", 5.0, "-ms", 45, "-map", 20, "-map-cells", 256, 128,
                 "-k", base])
    got = [read_vti(f) for f in files(base)]
    cycles = [int(g["field"]["CYCLE"][0]) for g in got]
    assert cycles == sorted(set(range(0, A["ti"] + 1, 20)) | {A["ti"]}) and 20 in cycles
    sz = A["sizes"]
    npts = sz["global_NE"] * sz["NQ"]
    c = 2 * 9 + 8
    bound = ((sz["NQ"] + c) + (sz["global_NE"] + c)) * 2.0 ** -52 * A["diag"]["mass"]
    for g in got:
        assert g["whole_extent"] == [0, 256, 0, 128, 0, 0] and g["origin"] == [0.0, 0.0, 0.0] and g["spacing"] == [7.0 / 256, 3.0 / 128, 1.0]
        assert g["cell"]["n"].shape == (256 * 128,)
        assert g["cell"]["n"].sum() + g["field"]["OUTSIDE"][0] + g["field"]["N_EXCLUDED"][0] == npts
    assert got[-1]["field"]["N_EXCLUDED"][0] == 0
    assert abs(got[-1]["cell"]["mass"].sum() + got[-1]["field"]["OUTSIDE"][2] - A["diag"]["mass"]) <= bound
