"""`laghos -prof N` through host_lib's sim object and the `laghos` executable (the pattern of tests/test_gpu_history_driver.py):
which files are written and what they hold, that the run itself is untouched, that a restarted run writes the files of its
segment byte for byte, and that bad option values are refused before any GPU work.

`-ms N` takes N + 1 steps as the reference's loop does: `-ms 6 -prof 2` writes cycles 0, 2, 4, 6 and the last one, 7; the
state of cycle 6 is the final state of the same run with `-ms 5`.  The exact Sedov columns are lgh_sedov_eval on the GPU against
context.sedov_eval_point on the host at the printed xi: 1e-11, skipping radii within 1e-12 of the shock, which is what
tests/test_gpu_sedov.py holds the same pair of calls to."""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import profile_ref as pr
from test_sedov_exact import close_to

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "laghos_amd", "laghos")

SEDOV_2D = ["-p", 1, "-dim", 2, "-nx", 8, "-ny", 8, "-ok", 2, "-ot", 1, "-ms", 6]
CYCLES = (0, 2, 4, 6, 7)


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
        return dict(t=sim.t, ti=sim.ti, fp=sim.fingerprint(), repeats=sim.repeats, sizes=sim.sizes(), look=look(sim) if look else None)
    finally:
        sim.close()


def files(base):
    return sorted(glob.glob(base + "_profile_*.csv"))


def test_files_header_rows_and_exact_columns(tmp_path):
    from laghos_amd import context
    base = str(tmp_path / "out" / "run")
    hi = float(np.sqrt(2.0))      # the largest distance of a node of the unit square from the origin
    A = run_sim(SEDOV_2D + ["-prof", 2, "-k", base], look=lambda sim: sim.profile("r", 64, 0.0, hi, (0.0, 0.0)))
    assert [os.path.basename(f) for f in files(base)] == ["run_profile_%06d.csv" % c for c in CYCLES] and A["ti"] == 7
    npts = A["sizes"]["global_NE"] * A["sizes"]["NQ"]
    for cyc in CYCLES:
        head, columns, rows, _ = pr.read_profile(base + "_profile_%06d.csv" % cyc)
        assert head["cycle"] == cyc and head["axis"] == "r" and head["nbins"] == 64 and head["n_excluded"] == 0
        assert (head["origin_x"], head["origin_y"], head["origin_z"], head["lo"]) == (0.0, 0.0, 0.0, 0.0)
        assert abs(head["hi"] - hi) <= 4 * 2.0 ** -52 and head["hi"] >= 1.0     # (sqrt on the host, from the mesh's own corner node)
        assert columns == pr.FILE_COLUMNS + pr.EXACT_COLUMNS
        assert sum(r["n"] for r in rows) == npts and rows[0]["n"] == 0
        assert (head["t"] == 0.0) == (cyc == 0)
    # the rows are Sim.profile of the same state, byte for byte once formatted (the range is the file's own): the last file
    # against the final state, the file of cycle 6 against the final state of the run that ends there
    head, _, rows, lines = pr.read_profile(base + "_profile_000007.csv")
    assert head["t"] == A["t"]
    B = run_sim(SEDOV_2D + ["-ms", 5, "-k", base + "_b"], look=lambda sim: sim.profile("r", 64, head["lo"], head["hi"], (0.0, 0.0)))
    assert B["ti"] == 6
    for table, cyc in ((A["look"]["rows"], 7), (B["look"]["rows"], 6)):
        head, _, rows, lines = pr.read_profile(base + "_profile_%06d.csv" % cyc)
        for r in range(66):
            exact = [rows[r][k] for k in pr.EXACT_COLUMNS]
            assert pr.format_row(r, 64, head["lo"], head["hi"], table[r], exact) == lines[2 + r], (cyc, r)
    assert head["t"] == B["t"]
    # the exact solution at the printed xi and the file's time
    par = context.sedov_setup(2, 1.4, 1.0, 1.0, 0.0)        # (-E0 defaults to 1)
    shock = context.sedov_shock(par, head["t"])
    full = [r for r in rows if r["mass"] != 0.0]
    assert len(full) >= 32 and all(np.isnan(r["rho_exact"]) for r in rows if r["mass"] == 0.0)
    want = np.array([context.sedov_eval_point(par, head["t"], r["xi"]) for r in full])
    for i, k in enumerate(pr.EXACT_COLUMNS):
        assert close_to([r[k] for r in full], want[:, i], 1e-11, shock_r=shock[0], r=[r["xi"] for r in full]), k
    ahead = [r for r in full if r["xi"] > shock[0] * (1 + 1e-12)]
    assert len(ahead) >= 16 and all(r["rho_exact"] == 1.0 and r["v_exact"] == 0.0 for r in ahead)     # undisturbed gas ahead of the shock
    # cycle 0 has no exact solution yet
    assert all(np.isnan(r["p_exact"]) for r in pr.read_profile(base + "_profile_000000.csv")[2])


def test_the_run_is_untouched(tmp_path):
    outs = []
    for extra in ([], ["-prof", 2]):
        k = str(tmp_path / ("exe%d" % len(extra)) / "run")
        p = subprocess.run([EXE] + strs(SEDOV_2D + extra + ["-vs", 1, "-fp", "-k", k]), capture_output=True, text=True, timeout=120, cwd=ROOT)
        assert p.returncode == 0, p.stdout + p.stderr
        outs.append((p.stdout, k))
    clock = re.compile(r"^(.*(?: total time| total time \(seconds\)| rate \(.*\))): .*$")
    plain, with_prof = ([clock.sub(r"\1:", l) for l in o[0].splitlines()] for o in outs)
    assert any(l.startswith("step ") for l in plain) and len([l for l in plain if l.startswith("State fingerprint:")]) == 1
    assert [l for l in with_prof if l.startswith("Profiles:")] == [f"Profiles: 5 files, {outs[1][1]}_profile_*.csv"]
    assert [l for l in with_prof if not l.startswith("Profiles:")] == plain          # the fingerprint line among them
    assert len(files(outs[1][1])) == 5
    assert not files(outs[0][1]) and not os.path.exists(os.path.dirname(outs[0][1]))   # without -prof: no file, no directory


def test_restart_writes_its_segment_byte_for_byte(tmp_path):
    base, base2 = str(tmp_path / "a" / "run"), str(tmp_path / "b" / "run")
    A = run_sim(SEDOV_2D + ["-prof", 2, "-k", base])
    want = {c: open(base + "_profile_%06d.csv" % c, "rb").read() for c in CYCLES}
    opts = SEDOV_2D + ["-prof", 2, "-ckpt", 3, "-ckpt-keep", 0, "-k", base2]
    B = run_sim(opts)
    assert B["fp"] == A["fp"]
    for c in CYCLES:
        assert open(base2 + "_profile_%06d.csv" % c, "rb").read() == want[c], c
        os.remove(base2 + "_profile_%06d.csv" % c)
    # (`-restart latest` would take the checkpoint written after the last step: the one of cycle 3 is named, as tests/test_gpu_history_driver.py does)
    C = run_sim(opts + ["-restart", f"{base2}_restart/cycle_000003.lgr"])
    assert C["fp"] == A["fp"]
    # the files of its own segment and none for the checkpoint's state or before it; default range and origin as in the first run
    assert [os.path.basename(f) for f in files(base2)] == ["run_profile_000004.csv", "run_profile_000006.csv", "run_profile_000007.csv"]
    for c in (4, 6, 7):
        assert open(base2 + "_profile_%06d.csv" % c, "rb").read() == want[c], c


def test_1d_sod_along_x_and_3d_along_z(tmp_path):
    base = str(tmp_path / "sod")
    A = run_sim(["-p", 2, "-m", "data/segment01.mesh", "-rs", 3, "-ms", 30, "-prof", 10, "-prof-bins", 16, "-k", base])
    got = [pr.read_profile(f) for f in files(base)]
    cycles = [g[0]["cycle"] for g in got]
    assert cycles == sorted(set(range(0, A["ti"] + 1, 10)) | {A["ti"]}) and A["repeats"] > 0   # (repeated steps write no file)
    npts = A["sizes"]["global_NE"] * A["sizes"]["NQ"]
    for head, columns, rows, _ in got:
        assert head["axis"] == "x" and (head["lo"], head["hi"], head["nbins"]) == (0.0, 1.0, 16) and columns == pr.FILE_COLUMNS
        assert sum(r["n"] for r in rows) == npts and head["n_excluded"] == 0
        assert rows[0]["n"] == 0 and all(r["n"] > 0 for r in rows[1:-1])
        assert all(r["lo"] <= r["xi"] < r["hi"] for r in rows[1:-1])
    first, last = got[0][2], got[-1][2]
    assert abs(first[1]["rho"] - 1.0) < 1e-12 and abs(first[16]["rho"] - 0.1) < 1e-12              # Sod: rho = 1 | 0.1
    assert max(abs(r["v"]) for r in first[1:-1]) == 0.0 and max(r["v"] for r in last[1:-1]) > 0.0   # the fluid moves to the right
    # 3D, along z, explicit range that leaves the lowest layer of zones below lo
    base3 = str(tmp_path / "cube")
    look = lambda sim: sim.profile("z", 3, 0.25, 1.0)
    B = run_sim(["-p", 1, "-dim", 3, "-nx", 4, "-ny", 4, "-nz", 4, "-rs", 0, "-ok", 2, "-ot", 1, "-ms", 3, "-prof", 2, "-prof-axis", "z", "-prof-bins", 3,
                 "-prof-range", 0.25, 1.0, "-prof-origin", 0.5, 0.5, "-k", base3], look=look)
    assert [pr.read_profile(f)[0]["cycle"] for f in files(base3)] == [0, 2, 4]
    head, columns, rows, lines = pr.read_profile(files(base3)[-1])
    assert head["axis"] == "z" and (head["lo"], head["hi"], head["nbins"]) == (0.25, 1.0, 3) and columns == pr.FILE_COLUMNS
    assert (head["origin_x"], head["origin_y"], head["origin_z"]) == (0.5, 0.5, 0.0)
    npts = B["sizes"]["global_NE"] * B["sizes"]["NQ"]
    assert [r["n"] for r in rows] == [npts // 4] * 4 + [0]
    for r in range(5):
        assert pr.format_row(r, 3, 0.25, 1.0, B["look"]["rows"][r]) == lines[2 + r]


@pytest.mark.parametrize("bad,word", [(["-prof", 0], "-prof"), (["-prof", 2, "-prof-bins", 0], "-prof-bins"), (["-prof", 2, "-prof-bins", 5000], "-prof-bins"),
                                      (["-prof", 2, "-prof-axis", "z"], "-prof-axis"), (["-prof", 2, "-prof-range", 1, 1], "-prof-range"),
                                      (["-prof", 2, "-prof-axis", "q"], "-prof-axis"), (["-prof", 2, "-prof-origin"], "-prof-origin")],
                         ids=["prof-0", "bins-0", "bins-5000", "axis-z-in-2D", "range-1-1", "axis-q", "origin-empty"])
def test_bad_values_are_refused(bad, word, tmp_path):
    k = str(tmp_path / "out" / "run")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")     # no device is visible: a refusal cannot have needed one
    p = subprocess.run([EXE] + strs(SEDOV_2D + bad + ["-k", k]), capture_output=True, text=True, timeout=60, cwd=ROOT, env=env)
    assert p.returncode != 0 and word in p.stderr, p.stdout + p.stderr
    assert "Profiles:" not in p.stdout and not os.path.exists(os.path.dirname(k))


def test_unwritable_profile_ends_the_run(tmp_path):
    from laghos_amd import host_lib
    blocker = tmp_path / "file"
    blocker.write_text("x")
    with pytest.raises(RuntimeError):
        host_lib.Sim(strs(SEDOV_2D + ["-prof", 1, "-k", str(blocker / "run"), "-q"]))
    p = subprocess.run([EXE] + strs(SEDOV_2D + ["-prof", 1, "-k", str(blocker / "run")]), capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode != 0 and "-prof" in p.stderr and "Profiles:" not in p.stdout
