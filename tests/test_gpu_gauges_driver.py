"""`laghos -gauges N -gauge X [Y [Z]] [-gauge-file PATH] [-gauge-buffer M]` through host_lib's sim object and the `laghos` executable,
in the pattern of tests/test_gpu_loads_driver.py: which lines are written and what they hold, that the size of the device buffer
and the way the points are given change no byte, two ranks against one and a renumbered mesh against the plain one (the same bytes
wherever the runs hold the same state: same_state_same_bytes), that a restarted run leaves the file of the uninterrupted run byte
for byte, that every refusal comes before anything touches the GPU, and that a run without the option is untouched.

`-ms N` takes N + 1 steps as the reference's loop does, and the one cadence of the periodic outputs records the last step too:
`-ms 6 -gauges 2` writes cycles 0, 2, 4, 6 and the last one, 7; the state of cycle c is the final state of the same run with
`-ms c - 1`.  A line is compared with Sim.gauges of the same state through the text both give (%.17g: equal bits, equal bytes)."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import gauges_ref as gr
from derived_ref import TOL

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "laghos_amd", "laghos")
HEADER = "cycle t gauge x y z vx vy vz rho e p cs detj div_v"

SEDOV_3D = ["-p", 1, "-dim", 3, "-nx", 4, "-ny", 4, "-nz", 4, "-rs", 0, "-ok", 2, "-ot", 1]
SEDOV_2D = ["-p", 1, "-dim", 2, "-nx", 8, "-ny", 8, "-rs", 0, "-ok", 2, "-ot", 1]
SOD_1D = ["-p", 2, "-m", "data/segment01.mesh", "-rs", 3]
# the zone at the blast, a break point of every axis (it opens zone (2, 2, 2)), the far corner (the closed last intervals), an
# interior point, a point on a face between the two ranks' blocks
POINTS_3D = [(0.1, 0.07, 0.12), (0.5, 0.5, 0.5), (1.0, 1.0, 1.0), (0.3, 0.62, 0.9), (0.5, 0.2, 0.8), (0.81, 0.33, 0.05)]
POINTS_2D = [(0.05, 0.05), (0.5, 0.25), (1.0, 0.3), (0.77, 0.41), (0.0, 1.0)]
POINTS_1D = [(0.2,), (0.5,), (0.73,), (1.0,), (0.0,)]
CYCLES = [0, 2, 4, 6, 7]
EPS = np.finfo(np.float64).eps


def strs(a):
    return [str(x) for x in a]


def gauge_opts(points, every=2):
    out = ["-gauges", every]
    for X in points:
        out += ["-gauge"] + [repr(float(v)) for v in X]
    return out


def run_sim(args, points=None, nranks=1, rank=0, cid=None):
    """one leg: a fresh Sim stepped to its end; Sim.gauges(points) is evaluated on the final state"""
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
        return dict(t=sim.t, ti=sim.ti, fp=sim.fingerprint(), sizes=sim.sizes(), rows=sim.gauges(points) if points else None)
    finally:
        sim.close()


def at_start(args, points):
    from laghos_amd import host_lib
    sim = host_lib.Sim(strs(args) + ["-q"])
    try:
        return dict(t=sim.t, rows=sim.gauges(points))
    finally:
        sim.close()


def read_gauges(path):
    """(the raw lines without the header, the rows as dicts)"""
    from laghos_amd import host_lib
    lines = open(path).read().splitlines(keepends=True)
    assert lines[0] == HEADER + "\n" and all(l.endswith("\n") for l in lines)
    rows = []
    for l in lines[1:]:
        cells = l[:-1].split(" ")
        assert len(cells) == len(host_lib.GAUGES_FILE_COLUMNS)
        rows.append({k: (int(c) if k in ("cycle", "gauge") else float(c)) for k, c in zip(host_lib.GAUGES_FILE_COLUMNS, cells)})
    return lines[1:], rows


def text_of(cycle, leg):
    from laghos_amd import host_lib
    return host_lib.host_gauges_text(cycle, leg["t"], leg["rows"])


def initial_reference(zones, points):
    """the rows the initial condition gives at the points, from the host library's own discretisation and the numpy reference"""
    from laghos_amd import host_lib
    dim = len(zones)
    d = host_lib.host_disc("cartesian", 0, 2, 1, 1, zones=zones)
    breaks = [np.linspace(0.0, 1.0, n + 1) for n in zones]
    loc = [gr.locate_initial(breaks, X) for X in points]
    zone = np.array([sum(ijk[a] * int(np.prod(zones[:a])) for a in range(dim)) for ijk, _ in loc])
    T = gr.tables_at(2, 1, np.array([xi for _, xi in loc]))
    N, NE = int(d["h1map"].max()) + 1, int(np.prod(zones))
    m, r0 = gr.gauges_mass_reference(dim, NE, N, 3, 2, d["h1map"], d["S0"][:dim * N], d["rho0_l2"], zone, *T)
    return gr.gauges_reference(dim, NE, N, 3, 2, d["h1map"], d["S0"], d["gamma"], zone, *T, m)["rows"], r0, d


@gpu
@pytest.mark.parametrize("dim", [3, 2])
def test_lines_and_their_content(tmp_path, dim):
    base = str(tmp_path / "out" / "run")
    sedov, points, zones = (SEDOV_3D, POINTS_3D, (4, 4, 4)) if dim == 3 else (SEDOV_2D, POINTS_2D, (8, 8))
    n = len(points)
    A = run_sim(sedov + gauge_opts(points) + ["-ms", 6, "-k", base], points)
    assert A["ti"] == 7
    lines, rows = read_gauges(base + "_gauges.csv")
    assert [r["cycle"] for r in rows] == [c for c in CYCLES for _ in range(n)] and [r["gauge"] for r in rows] == list(range(n)) * len(CYCLES)
    # the lines are those of Sim.gauges on the same states
    legs = {7: A, 0: at_start(sedov + ["-ms", 6, "-k", base + "_0"], points)}
    for c in (2, 4, 6):
        legs[c] = run_sim(sedov + ["-ms", c - 1, "-k", base + f"_{c}"], points)
        assert legs[c]["ti"] == c and not os.path.exists(base + f"_{c}_gauges.csv")
    for i, c in enumerate(CYCLES):
        assert "".join(lines[i * n:(i + 1) * n]) == text_of(c, legs[c]), c
    assert len({r["t"] for r in rows}) == len(CYCLES) and rows[0]["t"] == 0.0
    # cycle 0: the gauge sits where it was asked for, at rest, with the density and energy of the initial condition in its zone
    ref, r0, d = initial_reference(zones, points)
    first = legs[0]["rows"]
    for g, X in enumerate(points):
        assert np.all(np.abs(first[g, :dim] - np.array(X)) <= 4 * EPS * np.maximum(np.abs(X), 1.0)), (g, X)
    assert not first[:, 3:6].any() and not first[:, dim:3].any()
    print(f"cycle 0: max |x - X| = {np.abs(first[:, :dim] - np.array(points)).max():.3e}, max |rho - rho0| = {np.abs(first[:, 6] - r0).max():.3e}")
    assert np.all(np.abs(first[:, 6] - r0) <= TOL * np.abs(d["rho0_l2"]).max()) and np.all(np.abs(r0 - 1.0) <= 1e-13)      # Sedov: rho0 = 1
    e_max = np.abs(d["S0"][2 * dim * (int(d["h1map"].max()) + 1):]).max()
    assert np.all(np.abs(first[:, 7] - ref[:, 7]) <= TOL * e_max)
    assert first[0, 7] > 0 and not first[2, 7]                          # the blast is in the zone at the origin, the far corner is cold
    last = np.array([[r[k] for k in ("rho", "e", "p", "detj")] for r in rows[-n:]])
    assert np.all(last[:, 0] > 0) and np.all(last[:, 3] > 0) and last[0, 2] > 0


@gpu
def test_sod_1d_and_the_interval_rule(tmp_path):
    """1D Sod on 16 zones: the gauge at the membrane x = 0.5 - a break point - belongs to the zone that STARTS there, the light side"""
    base = str(tmp_path / "out" / "run")
    n = len(POINTS_1D)
    A = run_sim(SOD_1D + gauge_opts(POINTS_1D, 3) + ["-ms", 9, "-k", base], POINTS_1D)
    lines, rows = read_gauges(base + "_gauges.csv")
    cycles = sorted({r["cycle"] for r in rows})
    assert cycles[0] == 0 and cycles[-1] == A["ti"] and all(c % 3 == 0 for c in cycles[:-1]) and len(rows) == n * len(cycles)
    assert "".join(lines[-n:]) == text_of(A["ti"], A)
    start = at_start(SOD_1D + ["-ms", 9, "-k", base + "_0"], POINTS_1D)
    assert "".join(lines[:n]) == text_of(0, start)
    first = start["rows"]
    assert np.all(np.abs(first[:, 0] - np.array([X[0] for X in POINTS_1D])) <= 4 * EPS) and not first[:, 1:6].any()
    assert np.all(np.abs(first[:, 6] - np.array([1.0, 0.1, 0.1, 0.1, 1.0])) <= 1e-13)      # rho0 = 1 | 0.1 (laghos.cpp:1189)
    assert np.all(np.abs(first[:, 8] - np.array([1.0, 0.1, 0.1, 0.1, 1.0])) <= 1e-13)      # p = (gamma - 1) rho e: 1 | 0.1


@gpu
def test_buffer_size_and_gauge_file_change_no_byte(tmp_path):
    opts = SEDOV_3D + ["-ms", 6]
    b0, b1, b2, b3 = (str(tmp_path / k / "run") for k in "abcd")
    run_sim(opts + gauge_opts(POINTS_3D, 1) + ["-k", b0])
    want = open(b0 + "_gauges.csv", "rb").read()
    assert len(want.splitlines()) == 1 + 8 * len(POINTS_3D)
    for buf, b in ((2, b1), (3, b2)):                                    # 8 samples: full buffers and a rest of 0 and of 2
        run_sim(opts + gauge_opts(POINTS_3D, 1) + ["-gauge-buffer", buf, "-k", b])
        assert open(b + "_gauges.csv", "rb").read() == want, buf
    path = tmp_path / "points.txt"
    with open(path, "w") as f:
        f.write("# gauges of the test\n\n")
        for X in POINTS_3D[2:]:
            f.write("  " + "\t".join(repr(float(v)) for v in X) + "   # a point\n")
        f.write("   \n#\n")
    run_sim(opts + gauge_opts(POINTS_3D[:2], 1) + ["-gauge-file", str(path), "-k", b3])        # the command line's first, then the file's
    assert open(b3 + "_gauges.csv", "rb").read() == want


@gpu
def test_restart_leaves_the_file_of_the_uninterrupted_run(tmp_path):
    base, base2 = str(tmp_path / "a" / "run"), str(tmp_path / "b" / "run")
    n = len(POINTS_3D)
    opts = SEDOV_3D + gauge_opts(POINTS_3D) + ["-ms", 6]
    A = run_sim(opts + ["-k", base])
    want = open(base + "_gauges.csv", "rb").read()
    ck = opts + ["-ckpt", 3, "-ckpt-keep", 0, "-k", base2]
    B = run_sim(ck)
    assert B["fp"] == A["fp"] and open(base2 + "_gauges.csv", "rb").read() == want
    C = run_sim(ck + ["-restart", f"{base2}_restart/cycle_000003.lgr"])
    assert C["fp"] == A["fp"] and open(base2 + "_gauges.csv", "rb").read() == want
    # the file as a run killed inside cycle 6 leaves it: the lines of cycle 7 gone, the last line of cycle 6 cut
    lines = want.decode().splitlines(keepends=True)
    with open(base2 + "_gauges.csv", "w") as f:
        f.write("".join(lines[:1 + 4 * n - 1]) + lines[1 + 4 * n - 1][:40])
    C = run_sim(ck + ["-restart", f"{base2}_restart/cycle_000003.lgr"])
    assert C["fp"] == A["fp"] and open(base2 + "_gauges.csv", "rb").read() == want
    # ... and as a run killed right after its checkpoint of cycle 3 leaves it with the default buffer: drained before the piece was written
    with open(base2 + "_gauges.csv", "w") as f:
        f.write("".join(lines[:1 + 2 * n]))
    C = run_sim(ck + ["-restart", f"{base2}_restart/cycle_000003.lgr"])
    assert C["fp"] == A["fp"] and open(base2 + "_gauges.csv", "rb").read() == want
    # a checkpoint cycle that is a gauge cycle too: its sample is in the file before the piece exists
    b3 = str(tmp_path / "c" / "run")
    D = run_sim(SEDOV_3D + gauge_opts(POINTS_3D, 3) + ["-ms", 6, "-ckpt", 3, "-ckpt-keep", 0, "-k", b3])
    whole = open(b3 + "_gauges.csv", "rb").read()
    cut = whole.decode().splitlines(keepends=True)
    assert [int(l.split()[0]) for l in cut[1::n]] == [0, 3, 6, 7]
    with open(b3 + "_gauges.csv", "w") as f:
        f.write("".join(cut[:1 + 2 * n]))
    E = run_sim(SEDOV_3D + gauge_opts(POINTS_3D, 3) + ["-ms", 6, "-ckpt", 3, "-ckpt-keep", 0, "-k", b3, "-restart", f"{b3}_restart/cycle_000003.lgr"])
    assert E["fp"] == D["fp"] == A["fp"] and open(b3 + "_gauges.csv", "rb").read() == whole


def run_two_ranks(args, points):
    cid = (b"LGHLOCAL" + os.urandom(16).hex().encode()).ljust(128, b"\0")
    out, err = {}, {}

    def leg(rank):
        try:
            out[rank] = run_sim(args, points, nranks=2, rank=rank, cid=cid)
        except Exception as ex:  # noqa: BLE001 - reported below
            err[rank] = repr(ex)
    th = [threading.Thread(target=leg, args=(r,), daemon=True) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=150)
    assert not any(t.is_alive() for t in th) and not err, err
    return out


CG_TOL = 1e-8       # the driver's default -cgt: the relative residual at which the velocity and energy solves stop
COLS = ("cycle", "t", "gauge", "x", "y", "z", "vx", "vy", "vz", "rho", "e", "p", "cs", "detj", "div_v")


def same_state_same_bytes(b1, b2, nr, what):
    """The two -gauges files line by line against the two -hist files of the same runs, by the rule of tests/test_gpu_loads_driver.py:
    the lines of cycle 0 (the same initial state) have the same bytes, and so have the lines of every later cycle whose -hist rows
    have - a run on another rank count or numbering sums its CG scalars in another order, so its states and times differ in the
    last bits from the first step on, before a gauge is sampled at all.  There every value is held to the project's rule as
    it stands there: equal text, or 1e-9 of itself, or below 1e-15.  One departure, with its reason:

    The rule of the -loads test suits integrals, which are all of the size of their column.  A gauge is a point, and ahead of the
    blast what it holds of the two fields the run SOLVES for is what the solves leave behind when they stop at a relative residual
    of CG_TOL - digits no two runs share.  Measured on two ranks against one: vx = -1.4655039e-10 against -1.4654475e-10 at (0.9,
    0.9, 0.9) in cycle 2 (1.0e-4 of the value; the largest over the run by column: vx 5.7e-6, vy 7.9e-6, vz 3.3e-6, div_v 1.0e-4),
    e = 2.515278443867623e-14 against 2.515278447110588e-14 at (0.81, 0.33, 0.05) (1.3e-9; the largest e 1.4e-8, p 1.4e-8, cs
    1.9e-6), beside values of order one and more at the blast.  A solve that stops at CG_TOL of the scale of its field pins a value
    down to that, so the columns the solves reach have a floor of a tenth of it: vx, vy, vz may differ by 0.1 CG_TOL = 1e-9 of the
    largest velocity component among the gauges of the cycle, and div_v, e, p each by 1e-9 of the largest of its own column; cs is
    the square root of e, so it is cs^2 that may differ by 1e-9 of the largest cs^2.  A value at the size of its field is held as
    every other one.  t, x, y, z, rho and detj, which no solve reaches but through the positions, are held value by value
    (measured: at most 5.9e-13 of themselves).

    That the gauges give the same bits on the same state under another numbering and rank count is what tests/test_gpu_gauges.py
    holds them to."""
    l1, l2 = read_gauges(b1 + "_gauges.csv")[0], read_gauges(b2 + "_gauges.csv")[0]
    h1, h2 = ([l.split()[:2] + l.split()[3:] for l in open(b + "_history.csv").read().splitlines()[1:]] for b in (b1, b2))
    assert len(l1) == len(l2) == nr * len(CYCLES) and len(h1) == len(h2) == len(CYCLES)
    assert l1[:nr] == l2[:nr]
    same = [i for i in range(len(CYCLES)) if h1[i] == h2[i]]
    for i in same:
        assert l1[i * nr:(i + 1) * nr] == l2[i * nr:(i + 1) * nr], CYCLES[i]
    print(f"{what}: cycles with the same -hist row, and the same -gauges lines: {[CYCLES[i] for i in same]} of {CYCLES}")
    col = {k: j for j, k in enumerate(COLS)}
    vel = [col[k] for k in ("vx", "vy", "vz")]
    worst, bad = {k: 0.0 for k in COLS}, []
    for i in range(len(CYCLES)):
        A = np.array([[float(c) for c in l.split()] for l in l1[i * nr:(i + 1) * nr]])
        B = np.array([[float(c) for c in l.split()] for l in l2[i * nr:(i + 1) * nr]])
        assert np.array_equal(A[:, [0, 2]], B[:, [0, 2]])                          # the same cycles, the same gauges
        err, size = np.abs(A - B), np.maximum(np.abs(A), np.abs(B))
        ok = (err <= 1e-9 * size) | (np.abs(A) < 1e-15)                            # the rule of the -loads test, value by value
        floor = np.zeros(len(COLS))
        floor[vel] = 0.1 * CG_TOL * size[:, vel].max()
        for k in ("div_v", "e", "p"):
            floor[col[k]] = 0.1 * CG_TOL * size[:, col[k]].max()
        ok |= err <= floor
        cs = col["cs"]
        ok[:, cs] |= np.abs(A[:, cs] ** 2 - B[:, cs] ** 2) <= 0.1 * CG_TOL * (size[:, cs] ** 2).max()
        rel = np.where((np.abs(A) >= 1e-15) & (err > 0), err / np.maximum(size, 1e-300), 0.0)
        for j, k in enumerate(COLS):
            worst[k] = max(worst[k], float(rel[:, j].max()))
        bad += [(CYCLES[i], int(g), COLS[j], A[g, j], B[g, j]) for g, j in zip(*np.nonzero(~ok))]
    print(f"{what}: the largest difference of a value not below 1e-15, relative to itself, by column: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items() if v))
    assert not bad, bad


@gpu
def test_two_ranks_against_one(tmp_path):
    n = len(POINTS_3D)
    opts = SEDOV_3D + gauge_opts(POINTS_3D) + ["-gauge-buffer", 3, "-hist", 2, "-ms", 6, "-tf", 1e9]
    b1, b2 = str(tmp_path / "one" / "run"), str(tmp_path / "two" / "run")
    run_sim(opts + ["-k", b1])
    two = run_two_ranks(opts + ["-k", b2], POINTS_3D)
    assert two[0]["sizes"]["pgrid"] != (1, 1, 1) and two[0]["sizes"]["NE"] == 32
    assert sorted(os.listdir(os.path.dirname(b2))) == ["run_gauges.csv", "run_history.csv"]      # rank 0 writes, once
    # both ranks hold the rows the file ends with
    assert np.array_equal(two[0]["rows"].view(np.uint64), two[1]["rows"].view(np.uint64))
    assert open(b2 + "_gauges.csv").read().endswith(text_of(7, two[0]))
    same_state_same_bytes(b1, b2, n, "two ranks")


@gpu
def test_a_renumbered_2d_run_against_the_plain_run(tmp_path):
    n = len(POINTS_2D)
    opts = SEDOV_2D + gauge_opts(POINTS_2D) + ["-hist", 2, "-ms", 6]
    b1, b2 = str(tmp_path / "lex" / "run"), str(tmp_path / "ren" / "run")
    run_sim(opts + ["-k", b1])
    B = run_sim(opts + ["-renumber", "random", "-k", b2], POINTS_2D)
    assert open(b2 + "_gauges.csv").read().endswith(text_of(7, B))
    same_state_same_bytes(b1, b2, n, "-renumber random")


def many_points(n):
    return "".join(f"{(k + 0.5) / n!r} 0.5 0.5\n" for k in range(n))


def refusals(tmp_path):
    files = {}
    for name, text in (("empty.txt", ""), ("comments.txt", "# nothing\n\n   # here\n"), ("word.txt", "0.5 0.5 0.5\n0.5 abc 0.5\n"), ("four.txt", "0.1 0.2 0.3 0.4\n"),
                       ("glued.txt", "0.5,0.5,0.5\n"), ("nan.txt", "0.5 nan 0.5\n"), ("two.txt", "0.5 0.5\n"), ("outside.txt", "0.5 0.5 0.5\n0.5 1.5 0.5\n"),
                       ("many.txt", many_points(4097)), ("most.txt", many_points(4090)), ("some.txt", many_points(1000))):
        files[name] = str(tmp_path / name)
        with open(files[name], "w") as f:
            f.write(text)
    g = ["-gauges", "2"]
    return {
        "gauge-without-gauges": (["-gauge", "0.5", "0.5", "0.5"], "-gauge describes the gauges of the -gauges file: it needs -gauges"),
        "file-without-gauges": (["-gauge-file", files["some.txt"]], "-gauge-file describes the gauges of the -gauges file: it needs -gauges"),
        "buffer-without-gauges": (["-gauge-buffer", "8"], "-gauge-buffer describes the gauges of the -gauges file: it needs -gauges"),
        "no-point": (g, "-gauges records time series at gauges: it needs a point"),
        "gauges-0": (["-gauges", "0", "-gauge", "0.5", "0.5", "0.5"], "-gauges / --gauge-steps must be at least 1, got 0"),
        "gauges-no-value": (["-gauge", "0.5", "0.5", "0.5", "-gauges"], "missing value for -gauges"),
        "gauge-no-number": (g + ["-gauge", "-q"], "-gauge X [Y [Z]] needs one to three numbers"),
        "gauge-nan": (g + ["-gauge", "0.5", "nan", "0.5"], "-gauge 0.5 nan 0.5: the coordinates must be finite numbers"),
        "two-numbers-in-3D": (g + ["-gauge", "0.5", "0.5"], "-gauge 0.5 0.5: the point has 2 coordinates, the mesh has 3 dimensions"),
        "outside": (g + ["-gauge", "0.5", "0.5", "0.5", "-gauge", "0.5", "-0.001", "0.5"], "-gauge 0.5 -0.001 0.5: the point lies outside the initial mesh"),
        "above": (g + ["-gauge", "1.0000000000000002", "0.5", "0.5"], "-gauge 1.0000000000000002 0.5 0.5: the point lies outside the initial mesh"),
        "65-on-the-command-line": (g + [x for k in range(65) for x in ("-gauge", repr((k + 0.5) / 65), "0.5", "0.5")], "at most 64 gauges on the command line"),
        "buffer-0": (g + ["-gauge", "0.5", "0.5", "0.5", "-gauge-buffer", "0"], "-gauge-buffer M: the buffer holds at least 1 sample, got 0"),
        "buffer-trailing-characters": (g + ["-gauge", "0.5", "0.5", "0.5", "-gauge-buffer", "8abc"], "-gauge-buffer M: the buffer holds at least 1 sample, got 8abc"),
        "buffer-not-a-number": (g + ["-gauge", "0.5", "0.5", "0.5", "-gauge-buffer", "many"], "-gauge-buffer M: the buffer holds at least 1 sample, got many"),
        "buffer-too-large": (g + ["-gauge-file", files["some.txt"], "-gauge-buffer", "2797"], "-gauge-buffer 2797: 2797 samples of 1000 gauges need more than 256 MiB"),
        "file-missing": (g + ["-gauge-file", str(tmp_path / "none.txt")], "none.txt: cannot read the file"),
        "file-no-value": (g + ["-gauge-file"], "missing value for -gauge-file"),
        "file-empty": (g + ["-gauge-file", files["empty.txt"]], "empty.txt: the file holds no point"),
        "file-comments-only": (g + ["-gauge-file", files["comments.txt"]], "comments.txt: the file holds no point"),
        "file-word": (g + ["-gauge-file", files["word.txt"]], "word.txt line 2: malformed"),
        "file-four-numbers": (g + ["-gauge-file", files["four.txt"]], "four.txt line 1: malformed"),
        "file-commas": (g + ["-gauge-file", files["glued.txt"]], "glued.txt line 1: malformed"),
        "file-nan": (g + ["-gauge-file", files["nan.txt"]], "nan.txt line 1: the coordinates must be finite numbers"),
        "file-two-numbers-in-3D": (g + ["-gauge-file", files["two.txt"]], "two.txt line 1: the point has 2 coordinates, the mesh has 3 dimensions"),
        "file-outside": (g + ["-gauge-file", files["outside.txt"]], "outside.txt line 2: the point lies outside the initial mesh"),
        "file-4097": (g + ["-gauge-file", files["many.txt"]], "-gauges: at most 4096 gauges in all, got 4097"),
        "4097-in-all": (g + ["-gauge-file", files["most.txt"]] + [x for k in range(7) for x in ("-gauge", repr((k + 0.5) / 7), "0.5", "0.5")],
                        "-gauges: at most 4096 gauges in all, got 4097"),
    }


def test_refusals_come_before_the_gpu(tmp_path):
    """(every refusal is decided while the command line is read or right after the mesh is known: the executable gives it on a machine
    without a GPU too - this test needs none)"""
    import glob
    out = tmp_path / "out"
    for case, (extra, message) in refusals(tmp_path).items():
        args = strs(SEDOV_3D + ["-ms", 1, "-k", str(out / "run"), "-q"]) + extra
        p = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=60, cwd=ROOT)
        assert p.returncode != 0, case
        lines = [l for l in p.stderr.splitlines() if l.startswith("laghos: ")]
        assert len(lines) == 1 and message in lines[0], (case, p.stderr)
        assert not glob.glob(str(out / "*")), case                   # nothing was set up, nothing written
    # and in 1D and 2D the count of numbers is the mesh's
    for mesh, extra, message in ((SOD_1D, ["-gauge", "0.5", "0.5"], "the point has 2 coordinates, the mesh has 1 dimensions"),
                                 (SEDOV_2D, ["-gauge", "0.5"], "the point has 1 coordinates, the mesh has 2 dimensions"),
                                 (SEDOV_2D, ["-gauge", "0.5", "0.5", "0.5"], "the point has 3 coordinates, the mesh has 2 dimensions")):
        p = subprocess.run([EXE] + strs(mesh + ["-ms", 1, "-k", str(out / "run"), "-q", "-gauges", 1]) + extra, capture_output=True, text=True, timeout=60, cwd=ROOT)
        assert p.returncode != 0 and "laghos: " in p.stderr and message in p.stderr, p.stderr
        assert not glob.glob(str(out / "*"))


@gpu
def test_without_the_option_nothing_changes(tmp_path):
    outs = []
    n = len(POINTS_3D)
    for extra in ([], gauge_opts(POINTS_3D)):
        k = str(tmp_path / ("exe%d" % min(len(extra), 1)) / "run")
        p = subprocess.run([EXE] + strs(SEDOV_3D + ["-ms", 6] + extra + ["-vs", 1, "-fp", "-hist", 3, "-k", k]), capture_output=True, text=True, timeout=120, cwd=ROOT)
        assert p.returncode == 0, p.stdout + p.stderr
        outs.append((p.stdout, k))
    clock = re.compile(r"^(.*(?: total time| total time \(seconds\)| rate \(.*\))): .*$")
    plain, with_gauges = ([clock.sub(r"\1:", l) for l in o[0].splitlines()] for o in outs)
    assert any(l.startswith("step ") for l in plain) and len([l for l in plain if l.startswith("State fingerprint:")]) == 1
    assert [l for l in with_gauges if l.startswith("Gauges:")] == [f"Gauges: {outs[1][1]}_gauges.csv, 5 cycles x {n} gauges"]
    assert [l for l in with_gauges if not l.startswith("Gauges:")] == [l.replace("exe0", "exe1") for l in plain]
    assert sorted(os.listdir(os.path.dirname(outs[0][1]))) == ["run_history.csv"]
    assert sorted(os.listdir(os.path.dirname(outs[1][1]))) == ["run_gauges.csv", "run_history.csv"]
    assert open(outs[0][1] + "_history.csv", "rb").read() == open(outs[1][1] + "_history.csv", "rb").read()
    assert len(read_gauges(outs[1][1] + "_gauges.csv")[1]) == 5 * n
