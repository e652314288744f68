"""`laghos -loads N [-loads-plane AXIS K]` through host_lib's sim object and the `laghos` executable: which lines are written and
what they hold, two ranks against one and a renumbered mesh against the plain one (the same bytes wherever the runs hold the same
state: same_state_same_bytes), that a restarted run leaves the file of the uninterrupted run byte for byte, and that a run without
the option is untouched.

`-ms N` takes N + 1 steps as the reference's loop does, and the one cadence of the periodic outputs records the last step too:
`-ms 6 -loads 2` writes cycles 0, 2, 4, 6 and the last one, 7; the state of cycle c is the final state of the same run with
`-ms c - 1`.  A line is compared with Sim.loads of the same state through the text both give (%.17g: equal bits, equal bytes).

Volume: xn(surface) / dim against the `volume` column of `-hist` within the bound of tests/loads_ref.py (kappa and the sum of
|addend| from the numpy reference on the state of that cycle) plus the diagnostics' own sum bound (tests/test_gpu_diagnostics.py)."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import loads_ref as lr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "laghos_amd", "laghos")
HEADER = "cycle t name n area fx fy fz pa p_mean power flux xn p_min p_max"

SEDOV_3D = ["-p", 1, "-dim", 3, "-nx", 4, "-ny", 4, "-nz", 4, "-rs", 0, "-ok", 2, "-ot", 1]
SEDOV_2D = ["-p", 1, "-dim", 2, "-nx", 8, "-ny", 8, "-rs", 0, "-ok", 2, "-ot", 1]
NAMES_3D = ["surface", "x0", "x1", "y0", "y1", "z0", "z1", "plane_z2"]
CYCLES = [0, 2, 4, 6, 7]


def strs(a):
    return [str(x) for x in a]


def run_sim(args, look=None, nranks=1, rank=0, cid=None):
    """one leg: a fresh Sim stepped to its end; look(sim) is evaluated on the final state"""
    from laghos_amd import host_lib
    sim = host_lib.Sim(strs(args) + ["-q"], nranks=nranks, rank=rank, nccl_id=cid)
    try:
        if nranks > 1:
            sim.enable_timers(False)
        rc = 1
        while rc == 1:
            rc = sim.step()
        assert rc == 0, "a step failed"
        sim.sync()
        return dict(t=sim.t, ti=sim.ti, fp=sim.fingerprint(), sizes=sim.sizes(), look=look(sim) if look else None, state=sim.state())
    finally:
        sim.close()


def read_loads(path):
    """(the raw lines without the header, the rows as dicts)"""
    from laghos_amd import host_lib
    lines = open(path).read().splitlines(keepends=True)
    assert lines[0] == HEADER + "\n" and all(l.endswith("\n") for l in lines)
    rows = []
    for l in lines[1:]:
        cells = l[:-1].split(" ")
        assert len(cells) == len(host_lib.LOADS_FILE_COLUMNS)
        rows.append({k: (c if k == "name" else (int(c) if k in ("cycle", "n") else float(c))) for k, c in zip(host_lib.LOADS_FILE_COLUMNS, cells)})
    return lines[1:], rows


def text_of(cycle, t, p):
    from laghos_amd import host_lib
    return host_lib.host_loads_text(cycle, t, p["names"], p["rows"])


def test_lines_and_their_content(tmp_path):
    from laghos_amd import host_lib
    base = str(tmp_path / "out" / "run")
    look = lambda sim: sim.loads([("z", 2)])
    opts = SEDOV_3D + ["-loads", 2, "-loads-plane", "z", 2, "-hist", 2]
    A = run_sim(opts + ["-ms", 6, "-k", base], look=look)
    assert A["ti"] == 7 and A["look"]["names"] == NAMES_3D
    lines, rows = read_loads(base + "_loads.csv")
    nr = 2 * 3 + 2
    assert [r["cycle"] for r in rows] == [c for c in CYCLES for _ in range(nr)] and [r["name"] for r in rows] == NAMES_3D * len(CYCLES)
    # the rows are those of Sim.loads on the same states
    legs = {7: A}
    for c in (2, 4, 6):
        legs[c] = run_sim(SEDOV_3D + ["-ms", c - 1, "-k", base + f"_{c}"], look=look)
        assert legs[c]["ti"] == c and not os.path.exists(base + f"_{c}_loads.csv")
    sim = host_lib.Sim(strs(SEDOV_3D + ["-ms", 6, "-k", base + "_0", "-q"]))
    try:
        legs[0] = dict(t=sim.t, look=look(sim), state=sim.state(), sizes=sim.sizes())
    finally:
        sim.close()
    for i, c in enumerate(CYCLES):
        assert "".join(lines[i * nr:(i + 1) * nr]) == text_of(c, legs[c]["t"], legs[c]["look"]), c
        assert legs[c]["look"]["n_excluded"] == 0
    # what the rows say: 16 faces of 4 x 4 points a wall, the plane as many; the faces of plane z = 2 look down
    last = rows[-nr:]
    assert [r["n"] for r in last] == [6 * 256] + [256] * 7
    assert abs(last[0]["area"] - 6.0) < 1e-6 and all(abs(r["area"] - 1.0) < 1e-6 for r in last[1:7]) and abs(last[7]["area"] - 1.0) < 0.05
    assert last[7]["fz"] < 0 < last[7]["pa"] and last[5]["fz"] < 0 < last[6]["fz"] and last[1]["fx"] < 0 < last[2]["fx"]
    assert all(r["p_min"] <= r["p_mean"] <= r["p_max"] for r in last) and rows[0]["power"] == 0.0 and rows[0]["flux"] == 0.0    # cycle 0: at rest
    # the volume of -hist
    hist = [l.split() for l in open(base + "_history.csv").read().splitlines()[1:]]
    assert [int(h[0]) for h in hist] == CYCLES
    d = lr.case_data((4, 4, 4), 2, 1)
    sz = A["sizes"]
    for h, c in zip(hist, CYCLES):
        surf = rows[CYCLES.index(c) * nr]
        fp = lr.FacePoints(d, S=legs[c]["state"], rho=np.ones(d["rho"].size), gamma=d["gamma"])
        bf = lr.boundary_faces(d)
        ref = lr.loads_reference(fp, np.concatenate([bf, np.zeros((len(bf), 1), np.int32)], 1), 1)
        vol = float(h[6])
        terms = (sz["NQ"] + 3 * 27 + 8) + (sz["global_NE"] + 3 * 27 + 8)
        b = lr.bound(3, d["D"], d["L"], ref["kappa"][0], ref["abs"][0, 8]) + 3 * terms * lr.EPS * vol
        print(f"cycle {c}: |xn / 3 - volume| = {abs(surf['xn'] / 3 - vol):.3e}, bound / 3 = {b / 3:.3e}")
        assert abs(surf["xn"] - 3 * vol) <= b and abs(ref["rows"][0, 8] - surf["xn"]) <= b


def run_two_ranks(args):
    cid = (b"LGHLOCAL" + os.urandom(16).hex().encode()).ljust(128, b"\0")
    out, err = {}, {}

    def leg(rank):
        try:
            out[rank] = run_sim(args, look=lambda sim: sim.loads([("z", 2)]), nranks=2, rank=rank, cid=cid)
        except Exception as ex:  # noqa: BLE001 - reported below
            err[rank] = repr(ex)
    th = [threading.Thread(target=leg, args=(r,), daemon=True) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=150)
    assert not any(t.is_alive() for t in th) and not err, err
    return out


def same_state_same_bytes(b1, b2, nr, what):
    """The two -loads files line by line against the two -hist files of the same runs: the lines of cycle 0 (the same initial state)
    have the same bytes, and so have the lines of every later cycle whose -hist rows have - a run on another rank count or
    numbering sums its CG scalars in another order, so its states, its times and its -hist rows differ in the last bits from
    the first step on, before lgh_loads is called at all (measured: t of cycle 2 0.0050360111814557653 against
    0.005036011181455767, fx of the surface -1.4825878508712929 against -1.4825878508712922).  That lgh_loads gives the same bits on
    the same state under another numbering and rank count is what tests/test_gpu_loads.py holds it to."""
    l1, l2 = read_loads(b1 + "_loads.csv")[0], read_loads(b2 + "_loads.csv")[0]
    # (without the dt column: the time-step estimate is a reduction of its own and no part of the state)
    h1, h2 = ([l.split()[:2] + l.split()[3:] for l in open(b + "_history.csv").read().splitlines()[1:]] for b in (b1, b2))
    assert len(l1) == len(l2) == nr * len(CYCLES) and len(h1) == len(h2) == len(CYCLES)
    assert l1[:nr] == l2[:nr]     # (the -hist row of cycle 0 need not agree: lgh_diagnostics sums over the ranks to its bound, not to the bit)
    same = [i for i in range(len(CYCLES)) if h1[i] == h2[i]]
    for i in same:
        assert l1[i * nr:(i + 1) * nr] == l2[i * nr:(i + 1) * nr], CYCLES[i]
    print(f"{what}: cycles with the same -hist row, and the same -loads lines: {[CYCLES[i] for i in same]} of {CYCLES}")
    for a, b in zip(l1, l2):                                      # the same rows, the same counts, and values that agree as the states do
        ca, cb = a.split(), b.split()
        assert ca[0] == cb[0] and ca[2:4] == cb[2:4]
        for x, y in zip(ca[4:], cb[4:]):
            assert x == y or abs(float(x) - float(y)) <= 1e-9 * max(abs(float(x)), abs(float(y)), 1e-30) or abs(float(x)) < 1e-15


def test_two_ranks_against_one(tmp_path):
    opts = SEDOV_3D + ["-loads", 2, "-loads-plane", "z", 2, "-hist", 2, "-ms", 6, "-tf", 1e9]
    b1, b2 = str(tmp_path / "one" / "run"), str(tmp_path / "two" / "run")
    run_sim(opts + ["-k", b1])
    two = run_two_ranks(opts + ["-k", b2])
    assert two[0]["sizes"]["pgrid"] != (1, 1, 1) and two[0]["sizes"]["NE"] == 32
    assert sorted(os.listdir(os.path.dirname(b2))) == ["run_history.csv", "run_loads.csv"]      # rank 0 writes, once
    # both ranks hold the rows the file ends with
    assert np.array_equal(two[0]["look"]["rows"].view(np.uint64), two[1]["look"]["rows"].view(np.uint64))
    assert open(b2 + "_loads.csv").read().endswith(text_of(7, two[0]["t"], two[0]["look"]))
    same_state_same_bytes(b1, b2, 8, "two ranks")


def test_a_renumbered_2d_run_against_the_plain_run(tmp_path):
    opts = SEDOV_2D + ["-loads", 2, "-loads-plane", "x", 3, "-loads-plane", "y", 8, "-hist", 2, "-ms", 6]
    b1, b2 = str(tmp_path / "lex" / "run"), str(tmp_path / "ren" / "run")
    look = lambda sim: sim.loads([("x", 3), ("y", 8)])
    run_sim(opts + ["-k", b1])
    B = run_sim(opts + ["-renumber", "random", "-k", b2], look=look)
    lines, rows = read_loads(b1 + "_loads.csv")
    assert [r["name"] for r in rows[:7]] == ["surface", "x0", "x1", "y0", "y1", "plane_x3", "plane_y8"] and len(rows) == 7 * len(CYCLES)
    assert [r["n"] for r in rows[:7]] == [4 * 8 * 4] + [8 * 4] * 6
    assert all(r["fz"] == 0.0 for r in rows)
    assert open(b2 + "_loads.csv").read().endswith(text_of(7, B["t"], B["look"]))
    same_state_same_bytes(b1, b2, 7, "-renumber random")


def test_restart_leaves_the_file_of_the_uninterrupted_run(tmp_path):
    base, base2 = str(tmp_path / "a" / "run"), str(tmp_path / "b" / "run")
    opts = SEDOV_3D + ["-loads", 2, "-loads-plane", "z", 2, "-ms", 6]
    A = run_sim(opts + ["-k", base])
    want = open(base + "_loads.csv", "rb").read()
    ck = opts + ["-ckpt", 3, "-ckpt-keep", 0, "-k", base2]
    B = run_sim(ck)
    assert B["fp"] == A["fp"] and open(base2 + "_loads.csv", "rb").read() == want
    # the file as a run killed inside cycle 6 leaves it: the lines of cycle 7 gone, the last line of cycle 6 cut
    lines = want.decode().splitlines(keepends=True)
    with open(base2 + "_loads.csv", "w") as f:
        f.write("".join(lines[:1 + 4 * 8 - 1]) + lines[1 + 4 * 8 - 1][:40])
    C = run_sim(ck + ["-restart", f"{base2}_restart/cycle_000003.lgr"])
    assert C["fp"] == A["fp"]
    assert open(base2 + "_loads.csv", "rb").read() == want


def test_without_the_option_nothing_changes(tmp_path):
    outs = []
    for extra in ([], ["-loads", 2, "-loads-plane", "z", 2]):
        k = str(tmp_path / ("exe%d" % len(extra)) / "run")
        p = subprocess.run([EXE] + strs(SEDOV_3D + ["-ms", 6] + extra + ["-vs", 1, "-fp", "-hist", 3, "-k", k]), capture_output=True, text=True, timeout=120, cwd=ROOT)
        assert p.returncode == 0, p.stdout + p.stderr
        outs.append((p.stdout, k))
    clock = re.compile(r"^(.*(?: total time| total time \(seconds\)| rate \(.*\))): .*$")
    plain, with_loads = ([clock.sub(r"\1:", l) for l in o[0].splitlines()] for o in outs)
    assert any(l.startswith("step ") for l in plain) and len([l for l in plain if l.startswith("State fingerprint:")]) == 1
    assert [l for l in with_loads if l.startswith("Loads:")] == [f"Loads: {outs[1][1]}_loads.csv, 5 cycles x 8 rows"]
    assert [l for l in with_loads if not l.startswith("Loads:")] == [l.replace("exe0", "exe5") for l in plain]
    assert sorted(os.listdir(os.path.dirname(outs[0][1]))) == ["run_history.csv"]
    assert sorted(os.listdir(os.path.dirname(outs[1][1]))) == ["run_history.csv", "run_loads.csv"]
    assert open(outs[0][1] + "_history.csv", "rb").read() == open(outs[1][1] + "_history.csv", "rb").read()
    assert len(read_loads(outs[1][1] + "_loads.csv")[1]) == 5 * 8
