"""`laghos -hist N` through host_lib's sim object and once through the `laghos` executable: which rows are written, that the
run itself is untouched, what the rows say about conservation, and that a restarted run continues the file byte for byte.

The 2D Sedov and 3D Sedov Q3Q2 command lines are those of tests/test_gpu_restart_driver.py; `-ms N` takes N + 1 steps as the
reference's loop does.  Bounds: a total of NE NQ non-negative terms summed in two orders differs by at most
NE NQ 2^-52 (ie + ke); the `Energy  diff:` line prints three significant digits, so the value behind it is within half a
unit of the last one."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "laghos_amd", "laghos")
EPS = 2.0 ** -52

SEDOV_2D = ["-p", 1, "-m", "data/square01_quad.mesh", "-rs", 1, "-ok", 2, "-ot", 1]
SEDOV_3D = ["-p", 1, "-m", "data/cube01_hex.mesh", "-rs", 1, "-ok", 3, "-ot", 2]
SOD_1D = ["-p", 2, "-m", "data/segment01.mesh", "-rs", 3, "-ms", 30]
CASES = {"2D-Sedov": SEDOV_2D, "3D-Sedov-Q3Q2": SEDOV_3D}


def strs(a):
    return [str(x) for x in a]


def run_sim(args):
    """one leg: a fresh Sim stepped to its end"""
    from laghos_amd import host_lib
    sim = host_lib.Sim(strs(args) + ["-q"])
    try:
        while True:
            rc = sim.step()
            assert rc >= 0, "a step failed"
            if rc == 0:
                break
        sim.sync()
        sizes = sim.sizes()
        return dict(t=sim.t, dt=sim.dt, ti=sim.ti, rk=sim.rk_steps, e=sim.e_norm(), fp=sim.fingerprint(), repeats=sim.repeats,
                    energy=sim.energy(), diag=sim.diagnostics(), nterms=sizes["global_NE"] * sizes["NQ"])
    finally:
        sim.close()


def read_history(path):
    """(header line, list of rows as dicts of floats / ints, the raw lines)"""
    from laghos_amd import host_lib
    lines = open(path).read().splitlines(keepends=True)
    assert all(l.endswith("\n") for l in lines)
    ints = ("cycle", "rk_steps", "repeats", "detj_min_rank", "detj_min_zone", "n_inverted", "n_negative_e", "n_nonfinite")
    rows = []
    for l in lines[1:]:
        cells = l.split()
        assert len(cells) == len(host_lib.HISTORY_COLUMNS)
        rows.append({k: (int(c) if k in ints else float(c)) for k, c in zip(host_lib.HISTORY_COLUMNS, cells)})
    return lines[0][:-1], rows, lines


@pytest.mark.parametrize("case", list(CASES))
def test_rows_and_conservation(case, tmp_path):
    from laghos_amd import host_lib
    base = str(tmp_path / "out" / "run")
    A = run_sim(CASES[case] + ["-ms", 5, "-hist", 2, "-k", base])
    header, rows, _ = read_history(base + "_history.csv")
    assert header == host_lib.host_history_header()
    assert [r["cycle"] for r in rows] == [0, 2, 4, 6] and A["ti"] == 6
    assert rows[0]["t"] == 0.0 and rows[0]["d_total"] == 0.0 and rows[0]["rk_steps"] == 0
    last = rows[-1]
    assert (last["t"], last["dt"], last["cycle"], last["rk_steps"], last["repeats"]) == (A["t"], A["dt"], A["ti"], A["rk"], A["repeats"])
    # the last row is what Sim.diagnostics() gives for the final state
    for k in ("mass", "volume", "ie", "ke", "detj_min", "rho_max", "p_max", "v_max"):
        assert last[k] == A["diag"][k], k
    bound = A["nterms"] * EPS * (last["ie"] + last["ke"])
    print(f"{case}: total {last['total']!r}, Sim.energy() {A['energy']!r}, bound {bound:.3e}; d_total per row {[r['d_total'] for r in rows]}")
    assert last["total"] == last["ie"] + last["ke"] and abs(last["total"] - A["energy"]) <= bound
    for r in rows:
        assert r["mass"] == rows[0]["mass"]              # the same masses through the same sum: the same bits in every row
        assert r["n_inverted"] == 0 and r["n_nonfinite"] == 0 and r["detj_min"] > 0
        assert r["ie"] >= 0 and r["ke"] >= 0
    assert rows[-1]["ke"] > 0 and rows[-1]["v_max"] > 0


@pytest.mark.parametrize("case", list(CASES))
def test_the_run_is_untouched(case, tmp_path):
    opts = CASES[case] + ["-ms", 5]
    base = str(tmp_path / "sim" / "run")
    A = run_sim(opts + ["-k", base])
    assert not os.path.exists(base + "_history.csv") and not os.path.exists(str(tmp_path / "sim"))
    B = run_sim(opts + ["-hist", 1, "-k", base])
    for k in ("fp", "t", "dt", "e", "ti", "rk", "repeats"):
        assert A[k] == B[k], k
    _, rows, _ = read_history(base + "_history.csv")
    assert [r["cycle"] for r in rows] == list(range(0, A["ti"] + 1))
    # the executable: the same output apart from the History: line
    outs = []
    for extra in ([], ["-hist", 1]):
        k = str(tmp_path / ("exe%d" % len(extra)) / "run")
        p = subprocess.run([EXE] + strs(opts + extra + ["-vs", 1, "-fp", "-k", k]), capture_output=True, text=True, timeout=120, cwd=ROOT)
        assert p.returncode == 0, p.stdout + p.stderr
        outs.append((p.stdout, k))
    # (the timing block prints wall-clock seconds and rates, which no two runs share: their figures are blanked, the lines stay)
    clock = re.compile(r"^(.*(?: total time| total time \(seconds\)| rate \(.*\))): .*$")
    plain, with_hist = ([clock.sub(r"\1:", l) for l in o[0].splitlines()] for o in outs)
    assert any(l.endswith("total time:") for l in plain) and any(l.startswith("step ") for l in plain) and any(l.startswith("State fingerprint:") for l in plain)
    hist_lines = [l for l in with_hist if l.startswith("History:")]
    assert hist_lines == [f"History: {outs[1][1]}_history.csv, {A['ti'] + 1} rows"]
    assert [l for l in with_hist if not l.startswith("History:")] == plain
    assert not os.path.exists(outs[0][1] + "_history.csv") and not os.path.exists(os.path.dirname(outs[0][1]))
    # conservation against the figure the run itself prints: |energy_init - energy_final| to three digits
    m = re.search(r"^Energy  diff: (\d\.\d\de[+-]\d+)$", outs[1][0], re.M)
    assert m, outs[1][0]
    printed = float(m.group(1))
    half_unit = 0.005 * 10.0 ** int(m.group(1).split("e")[1])
    _, erows, _ = read_history(outs[1][1] + "_history.csv")
    last = erows[-1]
    slack = A["nterms"] * EPS * last["total"]
    print(f"{case}: Energy diff {printed:.2e}, |d_total| of the last row {abs(last['d_total']):.3e}, all rows {[r['d_total'] for r in erows]}")
    assert abs(abs(last["d_total"]) - printed) <= half_unit + slack
    assert erows == rows                                   # the executable wrote what the sim object wrote
    for r in erows:                                        # the bar the project holds `Energy diff` to (tests/test_gpu_pipeline.py), at every row
        assert abs(r["d_total"]) < 1e-4 * erows[0]["total"]


@pytest.mark.parametrize("case,ms,K", [("2D-Sedov", 6, 4), ("2D-Sedov", 6, 3), ("3D-Sedov-Q3Q2", 4, 3)], ids=["2D-K4", "2D-K3-odd", "3D-K3-odd"])
def test_restart_continues_the_file(case, ms, K, tmp_path):
    base = str(tmp_path / "out" / "run")
    path = base + "_history.csv"
    opts = CASES[case] + ["-ms", ms, "-hist", 2, "-ckpt", K, "-ckpt-keep", 0, "-k", base]
    B = run_sim(opts)
    b_bytes = open(path, "rb").read()
    _, rows, lines = read_history(path)
    last = B["ti"]
    assert [r["cycle"] for r in rows] == sorted(set(range(0, last + 1, 2)) | {last})
    stem = f"{base}_restart/cycle_{K:06d}.lgr"
    # the file is there: rows after cycle K are dropped and written again - the same bytes
    C = run_sim(opts + ["-restart", stem])
    assert C["fp"] == B["fp"] and C["ti"] == last
    assert open(path, "rb").read() == b_bytes
    # the file is gone: a new one with the header and the rows after cycle K (none for the checkpoint's own state)
    os.remove(path)
    C2 = run_sim(opts + ["-restart", stem])
    assert C2["fp"] == B["fp"]
    want = lines[0] + "".join(l for l, r in zip(lines[1:], rows) if r["cycle"] > K)
    assert open(path).read() == want
    assert K not in [r["cycle"] for r in read_history(path)[1]]


def test_1d_repeated_steps_write_no_row(tmp_path):
    base = str(tmp_path / "run")
    A = run_sim(SOD_1D + ["-hist", 1, "-k", base])
    assert A["repeats"] > 0
    _, rows, _ = read_history(base + "_history.csv")
    assert [r["cycle"] for r in rows] == list(range(0, A["ti"] + 1))   # one row per accepted step, none for a repeated one
    rep = [r["repeats"] for r in rows]
    print(f"1D Sod: {A['ti']} accepted steps, {A['rk']} RK steps, repeats per row {rep}, the sim's {A['repeats']}")
    assert all(a <= b for a, b in zip(rep, rep[1:])) and rep[0] == 0 and rep[-1] == A["repeats"]
    assert [r["rk_steps"] for r in rows] == [r["cycle"] + r["repeats"] for r in rows]
    assert all(r["pz"] == 0.0 and r["py"] == 0.0 for r in rows) and rows[-1]["n_nonfinite"] == 0


def test_unwritable_history_ends_the_run(tmp_path):
    from laghos_amd import host_lib
    blocker = tmp_path / "file"
    blocker.write_text("x")
    with pytest.raises(RuntimeError):
        host_lib.Sim(strs(SEDOV_2D + ["-ms", 2, "-hist", 1, "-k", str(blocker / "run"), "-q"]))
    p = subprocess.run([EXE] + strs(SEDOV_2D + ["-ms", 2, "-hist", 1, "-k", str(blocker / "run")]), capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode != 0 and "-hist" in p.stderr and "History:" not in p.stdout
