"""`laghos -peaks N [-peaks-arrival P]`: the running records of the driver through host_lib's sim object and the `laghos`
executable, on the meshes of tests/test_gpu_faces_driver.py (cube01_hex -rs 1, square01_quad -rs 1, -p 1).

The files check themselves: with -vs 1 -peaks 1 every cycle is dumped, and the record arrays of every dump must be what
tests/records_ref.py makes of the `pressure`, `density`, `specific_internal_energy` and `velocity` arrays of the dumps so far
at their TIMEs (the bars of records_ref.check_block: bit for bit, peak_speed within 4 eps).  Then the cadence (-peaks 3 -vs 2),
the arrival time for a threshold picked from a first run, a restart that must write the uninterrupted run's bytes, two ranks,
and that nothing changes without the option."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import records_ref as ref
from faces_ref import read_pvd
from vtu_reader import read_vtu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "laghos_amd", "laghos")

RUNS = {
    # id: (mesh options, slice, dim, the -pv-fields of the run and their names in a file)
    "3D": (["-p", 1, "-m", "data/cube01_hex.mesh", "-rs", 1], ("z", 1), 3, ["-pv-fields", "vorticity,detj"], ["vorticity", "detJ"]),
    "2D": (["-p", 1, "-m", "data/square01_quad.mesh", "-rs", 1], ("y", 3), 2, [], []),
}
STANDING = ["density", "velocity", "specific_internal_energy", "pressure"]
RECORD_NAMES = [n for n, _ in ref.DUMP_ARRAYS]


def strs(a):
    return [str(x) for x in a]


def dump_args(run, base, extra=()):
    mesh, (ax, K), _, fields, _ = RUNS[run]
    return strs(mesh + ["-k", base, "-paraview", "-pv-surface", "-pv-slice", ax, K] + fields + list(extra))


def set_dirs(run, base):
    ax, K = RUNS[run][1]
    return {"volume": base + "_paraview", "surface": base + "_surface", (ax, K): f"{base}_slice_{ax}{K}"}


def step_to_end(sim):
    rc = 1
    while rc == 1:
        rc = sim.step()
    assert rc == 0
    sim.sync()


def run_sim(args, which=()):
    """the sim stepped to its end; returns (final time, last cycle, Sim.records of the sets named)"""
    from laghos_amd import host_lib
    sim = host_lib.Sim(strs(args) + ["-q"])
    try:
        step_to_end(sim)
        return sim.t, sim.ti, {w: sim.records(w) for w in which}
    finally:
        sim.close()


def sample_of(f, dim):
    """(p, rho, e, v (dim, n)) as a dump file holds them"""
    A = f["arrays"]
    return A["pressure"], A["density"], A["specific_internal_energy"], np.ascontiguousarray(A["velocity"][:, :dim].T)


def block_of(f, want, arrival):
    """the record block of a dump file; what a file does not hold (p_last; arrival_time without a threshold) is taken from want"""
    got = want.copy()
    for name, col in ref.DUMP_ARRAYS + ((ref.ARRIVAL_ARRAY,) if arrival else ()):
        assert f["section"][name] == "PointData" and f["ncomp"][name] == 1, name
        got[col] = f["arrays"][name]
    return got


def point_data(f):
    return [n for n, s in f["section"].items() if s == "PointData"]


def replay_dir(d, cycles, dim, threshold, derived, faces, suffix=""):
    """every dump of directory d against the replay of the dumps before it; returns the last block and the times"""
    want, t_last, times = None, None, []
    for c in cycles:
        f = read_vtu(f"{d}/cycle_{c:06d}{suffix}.vtu")
        t = float(f["arrays"]["TIME"][0])
        assert int(f["arrays"]["CYCLE"][0]) == c
        p, rho, e, v = sample_of(f, dim)
        want = ref.update(want, p, rho, e, v, t, 0.0 if want is None else t - t_last, threshold, first=want is None)
        t_last = t
        times.append(t)
        # after the -pv-fields arrays; in a face dump before area_normal, which stays last
        names = STANDING + derived + RECORD_NAMES + (["arrival_time"] if threshold is not None else []) + (["area_normal"] if faces else [])
        assert point_data(f) == names, (d, c)
        ref.check_block(block_of(f, want, threshold is not None), want, dim, f"{d} cycle {c}")
    return want, times


def check_live(rec, want, t, threshold):
    """Sim.records against a block"""
    assert rec["time"] == t
    for name, col in ref.DUMP_ARRAYS + (ref.ARRIVAL_ARRAY,):
        if col == ref.SPEED:
            continue
        assert np.array_equal(ref.bits(rec[name]), ref.bits(want[col])), name
    if threshold is None:
        assert np.all(rec["arrival_time"] == -1.0)


@pytest.fixture(scope="module")
def first_runs(tmp_path_factory):
    """every cycle dumped, no threshold: the run the threshold is picked from"""
    out = {}
    for run in RUNS:
        base = str(tmp_path_factory.mktemp("first" + run) / "out" / "run")
        ax, K = RUNS[run][1]
        t, last, live = run_sim(dump_args(run, base, ["-ms", 4, "-vs", 1, "-peaks", 1]), ("volume", "surface", (ax, K)))
        out[run] = (base, t, last, live)
    return out


@pytest.mark.parametrize("run", list(RUNS))
def test_every_dump_holds_the_replay_of_the_dumps_before_it(run, first_runs):
    base, t_final, last, live = first_runs[run]
    _, _, dim, _, derived = RUNS[run]
    assert last == 5
    cycles = list(range(last + 1))
    for which, d in set_dirs(run, base).items():
        assert sorted(os.listdir(d)) == [f"cycle_{c:06d}.vtu" for c in cycles], d
        want, times = replay_dir(d, cycles, dim, None, derived, which != "volume")
        assert [float(t) for t, _ in read_pvd((base if which == "volume" else d) + ".pvd")] == times and times[-1] == t_final
        assert want.shape[1] > 0 and np.all(want[1] <= t_final)
        f = read_vtu(f"{d}/cycle_{last:06d}.vtu")
        rec = live[which]
        check_live(rec, want, t_final, None)                                  # Sim.records: the last dump
        for name, _ in ref.DUMP_ARRAYS:
            assert np.array_equal(ref.bits(rec[name]), ref.bits(f["arrays"][name])), (which, name)
    vol = replay_dir(base + "_paraview", cycles, dim, None, derived, False)[0]
    assert np.any(vol[1] > 0.0) and np.any(vol[1] == 0.0) and np.any(vol[2] > 0.0)   # peaks that came later, peaks at the start, impulse
    assert not os.path.exists(base + "_restart")                             # no checkpoint, no sidecar


@pytest.mark.parametrize("run", list(RUNS))
def test_arrival_time(run, first_runs, tmp_path):
    """a threshold between the least and the largest peak pressure of the first run's surface: some points cross, some do not"""
    base0, _, last, live0 = first_runs[run]
    _, (ax, K), dim, _, derived = RUNS[run]
    peak = live0["surface"]["peak_pressure"]
    P = float(0.5 * (peak.min() + peak.max()))
    assert peak.min() < P < peak.max()
    base = str(tmp_path / "out" / "run")
    t_final, last2, live = run_sim(dump_args(run, base, ["-ms", 4, "-vs", 1, "-peaks", 1, "-peaks-arrival", repr(P)]), ("volume", "surface", (ax, K)))
    assert last2 == last
    for which, d in set_dirs(run, base).items():
        want, _ = replay_dir(d, list(range(last + 1)), dim, P, derived, which != "volume")
        check_live(live[which], want, t_final, P)
        arr = live[which]["arrival_time"]
        crossed = live[which]["peak_pressure"] >= P
        assert np.all(arr[~crossed] == -1.0) and np.all(arr[crossed] >= 0.0)
        if which != (ax, K):
            assert crossed.any() and not crossed.all(), which
        # the other columns do not know of the threshold: the first run's bits
        for name, _ in ref.DUMP_ARRAYS:
            assert np.array_equal(ref.bits(live[which][name]), ref.bits(live0[which][name])), (which, name)


def test_1d_volume_records(tmp_path):
    """1D (the FA path, problem 2): the volume lattice of -paraview is the only material dump there"""
    base = str(tmp_path / "out" / "run")
    t_final, last, live = run_sim(["-p", 2, "-m", "data/segment01.mesh", "-rs", 3, "-k", base, "-paraview", "-ms", 12, "-vs", 1, "-peaks", 1,
                                   "-peaks-arrival", 0.5], ("volume",))
    assert 3 <= last <= 13                                                   # (-ms counts the repeated steps of the start too)
    want, times = replay_dir(base + "_paraview", list(range(last + 1)), 1, 0.5, [], False)
    check_live(live["volume"], want, t_final, 0.5)
    assert times[-1] == t_final and np.any(want[7] == 0.0) and np.any(want[7] == -1.0)    # Sod: p = 1 on the left, 0.1 on the right


def test_cadence(tmp_path):
    """-peaks 3 -vs 2 -ms 4 (cycles 1..5, dumps at 0, 2, 4 and the last): updates at exactly cycles 0, 2, 3, 4 and 5 - seen in the
    time of the last update after every step - and the records are the replay of the samples at those cycles with those dtr"""
    from laghos_amd import host_lib
    run, dim = "3D", 3
    base = str(tmp_path / "out" / "run")
    sim = host_lib.Sim(dump_args(run, base, ["-ms", 4, "-vs", 2, "-peaks", 3]) + ["-q"])
    try:
        R = sim.sizes()["D1D"] - 1

        def sample():
            d = sim.face_fields(R, "surface")
            return d["p"], d["rho"], d["e"], d["v"]

        want = ref.update(None, *sample(), 0.0, 0.0, first=True)
        check_live(sim.records("surface"), want, 0.0, None)
        t_last, updated, blocks = 0.0, [0], {0: want}
        while sim.step() == 1:
            c, t = sim.ti, sim.t
            rec = sim.records("surface")
            assert rec["time"] == sim.records("volume")["time"]               # one cadence for all sets
            if rec["time"] == t:
                updated.append(c)
                want = ref.update(want, *sample(), t, t - t_last)
                t_last = t
                blocks[c] = want
            else:
                assert rec["time"] == t_last
            check_live(rec, want, t_last, None)
            got = np.stack([rec[n] for n, _ in ref.DUMP_ARRAYS])
            ref.check_block(np.stack([got[0], got[1], got[2], want[3], got[3], got[4], got[5], want[7]]), want, dim, f"cycle {c}")
        assert sim.ti == 5 and updated == [0, 2, 3, 4, 5]
    finally:
        sim.close()
    d = base + "_surface"
    assert sorted(os.listdir(d)) == [f"cycle_{c:06d}.vtu" for c in (0, 2, 4, 5)]
    for c in (0, 2, 4, 5):                                                   # a dump never shows stale records
        f = read_vtu(f"{d}/cycle_{c:06d}.vtu")
        ref.check_block(block_of(f, blocks[c], False), blocks[c], dim, f"dump {c}")


# ---- restart ----------------------------------------------------------------------------------------------------------
def dump_files(base, run):
    out = {}
    for d in set_dirs(run, base).values():
        for name in os.listdir(d):
            out[os.path.join(d, name)] = open(os.path.join(d, name), "rb").read()
    for pvd in [base + ".pvd"] + [d + ".pvd" for w, d in set_dirs(run, base).items() if w != "volume"]:
        out[pvd] = open(pvd, "rb").read()
    return out


@pytest.mark.parametrize("N", [1, 2])
def test_restart_writes_the_same_files(N, tmp_path, first_runs):
    """-ms 6 -ckpt 3 (-vs 2: dumps at 0, 2, 4, 6, 7): the run restarted from cycle 3 writes the dumps of the uninterrupted one byte
    for byte; with -peaks 2 the checkpoint falls between the updates at 2 and 4, so dtr spans the restart"""
    run = "2D"
    peak = first_runs[run][3]["surface"]["peak_pressure"]
    P = repr(float(0.5 * (peak.min() + peak.max())))
    base = str(tmp_path / "pv" / "run")
    opts = dump_args(run, base, ["-ms", 6, "-vs", 2, "-peaks", N, "-peaks-arrival", P])
    run_sim(opts + ["-ckpt", 3, "-ckpt-keep", 0])
    rdir = base + "_restart"
    assert sorted(os.listdir(rdir)) == sorted([f"cycle_{c:06d}.lgr" + s for c in (3, 6, 7) for s in ("", ".rec")] + ["latest"])
    whole = dump_files(base, run)
    later = [p for p in whole if re.search(r"cycle_00000[4-7]\.vtu$", p) or p.endswith(".pvd")]
    assert len(later) == 3 * 3 + 3
    for p in later:
        os.remove(p)
    stamp = os.stat(f"{base}_surface/cycle_000000.vtu").st_mtime_ns
    ckpt = f"{rdir}/cycle_000003.lgr"
    # a restart without -peaks ignores the sidecar (and says so); with -peaks it needs the right one
    from laghos_amd import host_lib
    sc = host_lib.host_read_records_sidecar(ckpt + ".rec")
    assert sc["ti"] == 3 and sc["R"] == 2 and [t for t, _ in sc["sets"]] == ["volume", "surface", "slice_y3"]
    t2 = float(read_vtu(f"{base}_surface/cycle_000002.vtu")["arrays"]["TIME"][0])
    assert (sc["time"] == t2) == (N == 2) and sc["time"] >= t2               # -peaks 2: the last update before cycle 3 was at cycle 2
    for bad in (["-vr", 3], ["-peaks-arrival", "1e300"]):                    # (a later option overrides the earlier one)
        with pytest.raises(RuntimeError):
            host_lib.Sim(opts + strs(bad) + ["-restart", ckpt, "-q"])
    os.rename(ckpt + ".rec", ckpt + ".away")
    with pytest.raises(RuntimeError):
        host_lib.Sim(opts + ["-restart", ckpt, "-q"])
    os.rename(ckpt + ".away", ckpt + ".rec")
    assert not [p for p in later if os.path.exists(p)]                       # the refused restarts wrote nothing
    run_sim(opts + ["-restart", ckpt])
    again = dump_files(base, run)
    assert sorted(again) == sorted(whole)
    for p in whole:
        assert again[p] == whole[p], p
    assert os.stat(f"{base}_surface/cycle_000000.vtu").st_mtime_ns == stamp  # no cycle-0 dump on a restart


def test_checkpoint_keep_removes_the_sidecars_with_their_pieces(tmp_path):
    base = str(tmp_path / "pv" / "run")
    run_sim(strs(RUNS["2D"][0] + ["-k", base, "-pv-surface", "-ms", 5, "-vs", 100, "-peaks", 2, "-ckpt", 2, "-ckpt-keep", 1]))
    assert sorted(os.listdir(base + "_restart")) == ["cycle_000006.lgr", "cycle_000006.lgr.rec", "latest"]


def test_restart_without_peaks_ignores_the_sidecar(tmp_path):
    base = str(tmp_path / "pv" / "run")
    common = strs(RUNS["2D"][0] + ["-k", base, "-pv-surface", "-ms", 3, "-vs", 100])
    run_sim(common + ["-peaks", 1, "-ckpt", 2, "-ckpt-keep", 0])
    p = subprocess.run([EXE] + common + ["-restart", f"{base}_restart/cycle_000002.lgr"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout + p.stderr
    said = [l for l in p.stdout.splitlines() if "cycle_000002.lgr.rec" in l]
    assert len(said) == 1 and "ignores" in said[0] and not any(l.startswith("Peaks:") for l in p.stdout.splitlines())
    assert "peak_pressure" not in point_data(read_vtu(f"{base}_surface/cycle_000004.vtu"))


# ---- two ranks ----------------------------------------------------------------------------------------------------------
def test_two_ranks(tmp_path):
    """two ranks as threads on the LGHLOCAL communicator (as tests/test_gpu_faces_driver.py runs them): each rank's pieces against
    the replay of its own pieces; rank 0 has no face of the x = 4 plane and keeps an empty block for it"""
    from laghos_amd import host_lib
    dim, last, nranks = 3, 3, 2
    base = str(tmp_path / "r2" / "run")
    args = strs(["-dim", 3, "-nx", 8, "-ny", 4, "-nz", 4, "-Sx", 2, "-Sy", 1, "-Sz", 1, "-rs", 0, "-p", 1, "-ok", 2, "-ot", 1, "-pa", "-tf", 1e9, "-ms", last - 1,
                 "-vs", 1, "-paraview", "-pv-surface", "-pv-slice", "x", 4, "-peaks", 1, "-peaks-arrival", 0.05, "-k", base, "-q"])
    cid = (b"LGHLOCAL" + os.urandom(16).hex().encode()).ljust(128, b"\0")
    live, err = {}, {}

    def rank_main(rank):
        try:
            sim = host_lib.Sim(args, nranks=nranks, rank=rank, nccl_id=cid)
            try:
                sim.enable_timers(False)
                step_to_end(sim)
                live[rank] = (sim.t, {w: sim.records(w) for w in ("volume", "surface", ("x", 4))})
            finally:
                sim.close()
        except Exception as ex:  # noqa: BLE001 - reported below
            err[rank] = repr(ex)

    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(nranks)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in th) and not err, err
    cycles = list(range(last + 1))
    for which, tag in (("volume", "paraview"), ("surface", "surface"), (("x", 4), "slice_x4")):
        d = f"{base}_{tag}"
        txt = open(f"{d}/cycle_{last:06d}.pvtu").read()
        names = re.findall(r'<PDataArray type="Float64" Name="([^"]+)"', txt)
        assert names == ["Points"] + STANDING + RECORD_NAMES + ["arrival_time"] + (["area_normal"] if which != "volume" else [])
        for r in range(nranks):
            want, times = replay_dir(d, cycles, dim, 0.05, [], which != "volume", suffix=f".{r}")
            t_final, rec = live[r]
            assert times[-1] == t_final
            check_live(rec[which], want, t_final, 0.05)
    assert live[0][1][("x", 4)]["peak_pressure"].size == 0 and live[1][1][("x", 4)]["peak_pressure"].size == 16 * 9


# ---- without the option ---------------------------------------------------------------------------------------------
def tree(root):
    return sorted(os.path.relpath(os.path.join(dp, f), root) for dp, _, fs in os.walk(root) for f in fs)


def test_without_peaks_nothing_changes(tmp_path):
    """two runs of the same command without -peaks on this branch: the same files to the byte, the same lines, no line and no file
    of the records; with -peaks one line more, the sidecars more, and the files it does not touch the same to the byte.
    (That the parent commit writes these bytes too follows from no existing test changing.)"""
    outs = {}
    timing = re.compile(r"time|rate|FOM|megadofs|ParaView dumps|Face dumps|Checkpoints|History", re.I)   # (and lines that name the folder)
    for name, extra in (("base", []), ("again", []), ("peaks", ["-peaks", 2])):
        root = tmp_path / name
        args = dump_args("2D", str(root / "run"), ["-ms", 3, "-vs", 2, "-print", "-ckpt", 2, "-hist", 1] + extra)
        p = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert p.returncode == 0, p.stdout + p.stderr
        outs[name] = ([l for l in p.stdout.splitlines() if not timing.search(l)], tree(str(root)), str(root))
    lines, files, root = outs["base"]
    assert (lines, files) == outs["again"][:2] and len(lines) > 8
    assert not any(l.startswith("Peaks:") for l in lines) and not any(f.endswith(".rec") for f in files)
    for f in files:
        assert open(os.path.join(root, f), "rb").read() == open(os.path.join(outs["again"][2], f), "rb").read(), f
    lines_p, files_p, root_p = outs["peaks"]
    assert [l for l in lines_p if not l.startswith("Peaks:")] == lines and sum(l.startswith("Peaks:") for l in lines_p) == 1
    assert sorted(f for f in files_p if f not in files) == sorted(f + ".rec" for f in files if f.endswith(".lgr"))
    for f in files:
        if ".vtu" not in f:                                                  # everything but the dumps that now carry records
            assert open(os.path.join(root, f), "rb").read() == open(os.path.join(root_p, f), "rb").read(), f
