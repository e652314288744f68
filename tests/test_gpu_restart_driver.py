"""`laghos -ckpt N` / `-restart PATH` / `-fp` through host_lib's sim object (a fresh Sim per leg) and the `laghos` executable:
a restarted run must end on the SAME BITS as the run that was never interrupted (`==` on floats, np.array_equal on the
state), writing checkpoints must change nothing, and every checkpoint that does not belong to the command line is refused.

Legs of a case: A uninterrupted; A' = A again (the control: if A and A' differ the failure is the run-to-run
reproducibility of the step, not the restart, and is reported as such); B = A with -ckpt K; C = a fresh Sim with
-restart <stem of cycle K> and A's other options.

`-ms N` takes N + 1 steps as the reference's loop does (laghos.cpp:742-760), repeated ones included: the RK6 case repeats one
and ends on 6 accepted steps, and a run whose last step was the repeated one writes its final checkpoint for the state of the
last accepted step."""
import glob
import os
import re
import shutil
import struct
import subprocess
import threading

import numpy as np
import pytest

from fingerprint_ref import fp_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "laghos_amd", "laghos")

SEDOV_2D = ["-p", 1, "-m", "data/square01_quad.mesh", "-rs", 1, "-ok", 2, "-ot", 1, "-ms", 6]
CASES = {
    # id: (options, K; None = chosen from the run's repeated steps)
    "2D-Sedov": (SEDOV_2D, 4),
    "3D-Sedov-Q3Q2": (["-p", 1, "-m", "data/cube01_hex.mesh", "-rs", 1, "-ok", 3, "-ot", 2, "-ms", 4], 3),   # stress in registers, fused forces
    "3D-store-stress": (["-p", 1, "-m", "data/cube01_hex.mesh", "-rs", 1, "-ok", 2, "-ot", 1, "-ms", 4, "-store-stress"], 3),
    "2D-Gresho-RK2Avg": (["-p", 4, "-m", "data/square_gresho.mesh", "-rs", 0, "-ok", 3, "-ot", 2, "-s", 7, "-ms", 4], 2),
    "1D-Sod": (["-p", 2, "-m", "data/segment01.mesh", "-rs", 3, "-ms", 30], None),                            # repeats steps
    "2D-Sedov-RK6": (SEDOV_2D + ["-s", 6], 4),
}


def strs(a):
    return [str(x) for x in a]


def run_sim(args, nranks=1, rank=0, cid=None, trace=None):
    """one leg: a fresh Sim stepped to its end; what the comparisons need"""
    from laghos_amd import host_lib
    sim = host_lib.Sim(strs(args) + ["-q"], nranks=nranks, rank=rank, nccl_id=cid)
    try:
        if nranks > 1:
            sim.enable_timers(False)
        taken = 0
        while True:
            rc = sim.step()
            assert rc >= 0, "a step failed"
            if rc == 0:
                break
            taken += 1
            if trace is not None:
                trace.append((sim.ti, sim.repeats))
        sim.sync()
        return dict(S=sim.state(), t=sim.t, dt=sim.dt, ti=sim.ti, rk=sim.rk_steps, e=sim.e_norm(), fp=sim.fingerprint(),
                    repeats=sim.repeats, checks=sim.checks(), taken=taken)
    finally:
        sim.close()


def same(a, b, what):
    for k in ("t", "dt", "ti", "rk", "e", "fp", "repeats"):
        assert a[k] == b[k], (what, k, a[k], b[k])
    assert np.array_equal(a["S"].view(np.uint64), b["S"].view(np.uint64)), (what, "S")


def stem_of(base, ti):
    return f"{base}_restart/cycle_{ti:06d}.lgr"


def pieces(base):
    return sorted(os.listdir(base + "_restart"))


def tail_lines(out):
    """the lines of the executable's output that tell the end of a run"""
    keep = [l for l in out.splitlines() if l.startswith(("Energy  diff:", "State fingerprint:"))]
    steps = [l for l in out.splitlines() if l.startswith("step ")]
    return keep, steps[-1:]


@pytest.mark.parametrize("case", list(CASES))
def test_restart_ends_on_the_same_bits(case, tmp_path):
    opts, K = CASES[case]
    base = str(tmp_path / "out" / "run")
    trace = []
    A = run_sim(opts, trace=trace)
    A2 = run_sim(opts)
    same(A, A2, "A against A again: the step itself is not reproducible from run to run - not a restart failure")
    assert A["fp"] == fp_ref(A["S"])                      # one rank: Sim.fingerprint() is the fingerprint of S
    last = A["ti"]
    if K is None:
        # the latest accepted step that still has a repeated step after it (the middle of the run if there is none)
        rep_after = {ti: rep for ti, rep in trace}
        later = [ti for ti in range(1, last) if rep_after[ti] < A["repeats"]]
        K = later[-1] if later else max(1, last // 2)
        print(f"{case}: {last} accepted steps, {A['rk']} RK steps, repeats before / after cycle {K}: "
              f"{rep_after[K]} / {A['repeats'] - rep_after[K]}")
    assert 1 <= K < last
    # B: writing changes nothing; -ckpt-keep 0 keeps every piece
    B = run_sim(opts + ["-ckpt", K, "-ckpt-keep", 0, "-k", base])
    same(A, B, "B (with -ckpt) against A")
    written = [ti for ti in range(1, last + 1) if ti % K == 0 or ti == last]
    assert pieces(base) == sorted([f"cycle_{ti:06d}.lgr" for ti in written] + ["latest"])
    assert open(base + "_restart/latest").read() == f"cycle_{last:06d}.lgr\n"
    # C: the restart
    C = run_sim(opts + ["-restart", stem_of(base, K)])
    assert C["taken"] == last - K
    same(A, C, f"C (restart from cycle {K}) against A")
    # a restart from the checkpoint written after the last step takes no step and reports A's final values
    F = run_sim(opts + ["-restart", stem_of(base, last)])
    assert F["taken"] == 0
    same(A, F, "restart from the last checkpoint against A")
    # -restart latest = the named stem
    Lt = run_sim(opts + ["-restart", "latest", "-k", base])
    assert Lt["taken"] == 0
    same(F, Lt, "-restart latest against the named stem")
    # the executable: the same closing lines from the uninterrupted and the restarted run
    outs = []
    for extra in ([], ["-restart", stem_of(base, K)]):
        p = subprocess.run([EXE] + strs(opts + extra + ["-fp", "-vs", 1, "-k", str(tmp_path / "exe" / "run")]), capture_output=True,
                           text=True, timeout=120, cwd=ROOT)
        assert p.returncode == 0, p.stdout + p.stderr
        outs.append(p.stdout)
    closing, last_step = tail_lines(outs[0])
    assert len(closing) == 2 and len(last_step) == 1
    assert tail_lines(outs[1]) == (closing, last_step)
    assert closing[0] == f"State fingerprint: {A['fp'][0]:016X}{A['fp'][1]:016X} (cycle {last})" and closing[1].startswith("Energy  diff:")
    assert f"Restarting from {stem_of(base, K)}: cycle {K}," in outs[1] and "Restarting" not in outs[0]
    assert not os.path.exists(str(tmp_path / "exe"))      # neither run wrote anything


def test_keep_rule_and_latest(tmp_path):
    """-ckpt 2 on the 7 accepted steps of the 2D run writes cycles 2, 4, 6 and 7 (the last step); -ckpt-keep K leaves the K
    newest (default 2, 0 = all), `latest` names the newest, no .tmp is left"""
    want = {None: [6, 7], 0: [2, 4, 6, 7], 1: [7], 3: [4, 6, 7]}
    ref = None
    for keep, cycles in want.items():
        base = str(tmp_path / f"keep_{keep}" / "run")
        r = run_sim(SEDOV_2D + ["-ckpt", 2, "-k", base] + ([] if keep is None else ["-ckpt-keep", keep]))
        assert r["ti"] == 7
        assert pieces(base) == [f"cycle_{c:06d}.lgr" for c in cycles] + ["latest"], keep
        assert open(base + "_restart/latest").read() == "cycle_000007.lgr\n"
        assert not glob.glob(base + "_restart/*.tmp")
        if ref is None:
            ref = r
        same(ref, r, f"-ckpt-keep {keep}")


def test_keep_rule_removes_only_what_this_run_wrote(tmp_path):
    base = str(tmp_path / "run")
    os.makedirs(base + "_restart")
    for name in ("cycle_000001.lgr", "cycle_000099.lgr", "notes.txt"):
        open(os.path.join(base + "_restart", name), "w").write("somebody else's\n")
    run_sim(SEDOV_2D + ["-ckpt", 2, "-ckpt-keep", 1, "-k", base])
    assert pieces(base) == ["cycle_000001.lgr", "cycle_000007.lgr", "cycle_000099.lgr", "latest", "notes.txt"]


def test_checks_straddle_the_restart(tmp_path):
    """the 2D Sedov --checks run compares cycles 5 and 15; restarted from cycle 10 it still counts two checks and passes"""
    opts = ["-p", 1, "-m", "data/square01_quad.mesh", "-rs", 0, "-cgt", "1.e-14", "-chk", "-pa"]
    base = str(tmp_path / "run")
    A = run_sim(opts)
    assert A["checks"] == (2, True) and A["ti"] >= 15
    B = run_sim(opts + ["-ckpt", 10, "-ckpt-keep", 0, "-k", base])
    same(A, B, "B against A")
    from laghos_amd import host_lib
    S, t, c = np.empty(A["S"].size), np.empty(4), np.empty(4, dtype=np.int64)
    h = host_lib.host_read_checkpoint(stem_of(base, 10), S, t, c)
    assert (h["ti"], h["checks"], h["checks_ok"]) == (10, 1, 1) and h["state_fp"] == fp_ref(S)
    C = run_sim(opts + ["-restart", stem_of(base, 10)])
    same(A, C, "C against A")
    assert C["checks"] == (2, True)
    p = subprocess.run([EXE] + strs(opts + ["-restart", stem_of(base, 10)]), capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0 and "Check error" not in p.stdout, p.stdout + p.stderr


def test_options_that_differ_are_reported_and_the_command_line_wins(tmp_path):
    base = str(tmp_path / "run")
    run_sim(SEDOV_2D + ["-ckpt", 4, "-k", base])
    p = subprocess.run([EXE] + strs(SEDOV_2D + ["-restart", stem_of(base, 4), "-cfl", 0.25, "-cgm", 200, "-s", 3]), capture_output=True,
                       text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [l for l in p.stdout.splitlines() if l.startswith("Restart: ")]
    assert len(lines) == 3 and [l.split()[1] for l in lines] == ["-s", "-cfl", "-cgm"], lines


def test_checkpoint_between_steps_through_the_sim(tmp_path):
    """Sim.checkpoint(stem): a checkpoint of the sim as it stands; the restart continues to the same bits"""
    from laghos_amd import host_lib
    A = run_sim(SEDOV_2D)
    stem = str(tmp_path / "by" / "hand.lgr")
    sim = host_lib.Sim(strs(SEDOV_2D) + ["-q"])
    try:
        for _ in range(3):
            assert sim.step() == 1
        fp3 = sim.fingerprint()
        sim.checkpoint(stem)
        assert sim.fingerprint() == fp3
    finally:
        sim.close()
    S, t, c = np.empty(A["S"].size), np.empty(1), np.empty(1, dtype=np.int64)
    h = host_lib.host_read_checkpoint(stem, S, t, c)
    assert h["ti"] == 3 and h["state_fp"] == fp3 == fp_ref(S) and os.listdir(os.path.dirname(stem)) == ["hand.lgr"]
    same(A, run_sim(SEDOV_2D + ["-restart", stem]), "restart from Sim.checkpoint")


# ---- ParaView ---------------------------------------------------------------------------------------------------------
def test_paraview_collection_goes_on(tmp_path):
    base = str(tmp_path / "pv" / "run")
    opts = SEDOV_2D + ["-vs", 2, "-paraview", "-k", base]
    run_sim(opts + ["-ckpt", 4, "-ckpt-keep", 0])
    cycles = [0, 2, 4, 6, 7]
    entries = lambda: re.findall(r'file="run_paraview/cycle_(\d{6})\.vtu"', open(base + ".pvd").read())
    assert [int(c) for c in entries()] == cycles
    whole = {c: open(f"{base}_paraview/cycle_{c:06d}.vtu", "rb").read() for c in cycles}
    pvd = open(base + ".pvd").read()
    first = f"{base}_paraview/cycle_000000.vtu"
    stamp = os.stat(first).st_mtime_ns
    for c in (6, 7):
        os.remove(f"{base}_paraview/cycle_{c:06d}.vtu")
    os.remove(base + ".pvd")
    run_sim(opts + ["-restart", stem_of(base, 4)])
    assert [int(c) for c in entries()] == cycles              # before and after the restart, once each, in order
    assert open(base + ".pvd").read() == pvd
    assert os.stat(first).st_mtime_ns == stamp and open(first, "rb").read() == whole[0]   # no cycle-0 dump on a restart
    for c in (6, 7):
        assert open(f"{base}_paraview/cycle_{c:06d}.vtu", "rb").read() == whole[c], c


# ---- refusals ---------------------------------------------------------------------------------------------------------
def exe(args, timeout=120):
    return subprocess.run([EXE] + strs(args), capture_output=True, text=True, timeout=timeout, cwd=ROOT)


def test_ckpt_zero_is_refused_while_parsing(tmp_path):
    base = str(tmp_path / "run")
    p = exe(SEDOV_2D + ["-ckpt", 0, "-k", base])
    assert p.returncode != 0 and "-ckpt" in p.stderr and "at least 1" in p.stderr
    assert "Number of zones" not in p.stdout and not glob.glob(str(tmp_path / "*"))
    p = exe(SEDOV_2D + ["-ckpt-keep", -1, "-k", base])
    assert p.returncode != 0 and "-ckpt-keep" in p.stderr and "Number of zones" not in p.stdout


def test_restart_of_a_missing_file_is_refused(tmp_path):
    p = exe(SEDOV_2D + ["-restart", str(tmp_path / "nothing_restart" / "cycle_000004.lgr")])
    assert p.returncode != 0 and "cannot open" in p.stderr and "cycle_000004.lgr" in p.stderr and "step " not in p.stdout
    p = exe(SEDOV_2D + ["-restart", "latest", "-k", str(tmp_path / "nothing")])
    assert p.returncode != 0 and "latest" in p.stderr and "step " not in p.stdout


MISMATCHES = {
    # id: (options of the run that writes, options of the run that restarts)
    "rs": (["-rs", 1], ["-rs", 2]),
    "order": (["-ok", 2, "-ot", 1], ["-ok", 3, "-ot", 2]),
    "E0": (["-E0", 1], ["-E0", 2]),
    "renumber": (["-renumber", "mfem"], ["-renumber", "none"]),
}


@pytest.mark.parametrize("what", list(MISMATCHES))
def test_a_checkpoint_of_another_setup_is_refused(what, tmp_path):
    common = ["-p", 1, "-m", "data/cube01_hex.mesh", "-ms", 2]
    w, r = MISMATCHES[what]
    fill = lambda o: o + (["-rs", 1] if "-rs" not in o else []) + (["-ok", 2, "-ot", 1] if "-ok" not in o else [])
    base = str(tmp_path / "run")
    run_sim(common + fill(w) + ["-ckpt", 2, "-k", base])
    p = exe(common + fill(r) + ["-restart", stem_of(base, 2)])
    print(p.stderr.strip())
    assert p.returncode != 0 and "refused" in p.stderr and stem_of(base, 2) in p.stderr
    assert ("setup_fp" in p.stderr) and "step " not in p.stdout and "Restarting" not in p.stdout
    # and the run it belongs to takes it
    assert exe(common + fill(w) + ["-restart", stem_of(base, 2)]).returncode == 0


def test_an_altered_payload_is_caught_by_state_fp(tmp_path):
    """one bit of the state flipped after writing and the trailer made anew: the trailer passes, state_fp does not"""
    base = str(tmp_path / "run")
    run_sim(SEDOV_2D + ["-ckpt", 4, "-k", base])
    path = stem_of(base, 4)
    raw = bytearray(open(path, "rb").read())
    hb = int(bytes(raw).split(b"\n")[1].split()[1])
    raw[hb + 8 * 11] ^= 0x04
    body = bytes(raw[:-16])
    open(path, "wb").write(body + struct.pack("<2Q", *fp_ref(np.frombuffer(body, dtype=np.uint64))))
    p = exe(SEDOV_2D + ["-restart", path])
    assert p.returncode != 0 and "state_fp" in p.stderr and path in p.stderr and "step " not in p.stdout


def test_without_the_options_nothing_changes(tmp_path):
    """the parent's option set: the same output twice, no Checkpoints / fingerprint / Restart line, no _restart directory"""
    base = str(tmp_path / "run")
    outs = [exe(SEDOV_2D + ["-vs", 2, "-k", base]) for _ in range(2)]
    assert all(p.returncode == 0 for p in outs)
    timing = re.compile(r"time|rate|FOM|megadofs", re.I)
    lines = [[l for l in p.stdout.splitlines() if not timing.search(l)] for p in outs]
    assert lines[0] == lines[1] and len(lines[0]) > 8
    assert not any(w in outs[0].stdout for w in ("Checkpoint", "fingerprint", "Restart"))
    assert not glob.glob(str(tmp_path / "*"))


# ---- two ranks as threads in one process (the LGHLOCAL communicator, as tests/test_gpu_multiproc.py::_in_process) --------
def two_ranks(extra_by_rank, block=4, steps=6, dim=3):
    """both ranks' legs; a rank whose Sim is refused reports 'refused'"""
    mesh = ["-dim", dim, "-nx", 2 * block, "-ny", block, "-Sx", 2, "-Sy", 1] + (["-nz", block, "-Sz", 1] if dim == 3 else [])
    args = mesh + ["-rs", 0, "-p", 1, "-ok", 2, "-ot", 1, "-pa", "-tf", 1e9, "-ms", steps - 1, "-vs", 10 ** 9]
    cid = (b"LGHLOCAL" + os.urandom(16).hex().encode()).ljust(128, b"\0")
    out, err = {}, {}

    def rank_main(rank):
        try:
            out[rank] = run_sim(args + extra_by_rank[rank], nranks=2, rank=rank, cid=cid)
        except RuntimeError as ex:
            out[rank] = "refused" if "laghos_sim_create failed" in str(ex) else None
            if out[rank] is None:
                err[rank] = repr(ex)
        except Exception as ex:  # noqa: BLE001 - reported below
            err[rank] = repr(ex)

    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in th) and not err, err
    return out, args


def test_two_ranks(tmp_path, capfd):
    _two_ranks(tmp_path, capfd, 3)


def test_two_ranks_2d(tmp_path, capfd):
    """the same on two 2D blocks of 4 x 4 zones"""
    _two_ranks(tmp_path, capfd, 2)


def _two_ranks(tmp_path, capfd, dim):
    base = str(tmp_path / "two" / "run")
    run2 = lambda extra: two_ranks(extra, dim=dim)
    A, args = run2([[], []])
    assert A[0]["ti"] == 6 and A[0]["fp"] == A[1]["fp"]                     # the rank-ordered combination: one value for the run
    assert A[0]["fp"] != fp_ref(A[0]["S"]) and not np.array_equal(A[0]["S"], A[1]["S"])
    B, _ = run2([["-ckpt", 3, "-k", base]] * 2)
    for r in range(2):
        same(A[r], B[r], f"B against A, rank {r}")
    assert pieces(base) == ["cycle_000003.lgr.0", "cycle_000003.lgr.1", "cycle_000006.lgr.0", "cycle_000006.lgr.1", "latest"]
    assert open(base + "_restart/latest").read() == "cycle_000006.lgr\n"
    C, _ = run2([["-restart", stem_of(base, 3)]] * 2)
    for r in range(2):
        assert C[r]["taken"] == 3
        same(A[r], C[r], f"C against A, rank {r}")
    capfd.readouterr()
    # each rank given the other's piece
    d = base + "_restart/"
    for r in range(2):
        shutil.copy(d + f"cycle_000003.lgr.{r}", d + f"swapped.lgr.{1 - r}")
    R, _ = run2([["-restart", d + "swapped.lgr"]] * 2)
    assert R == {0: "refused", 1: "refused"}
    msg = capfd.readouterr().err
    assert "it is the piece of rank 1 of 2, this is rank 0 of 2" in msg and "swapped.lgr.0" in msg
    # pieces of two different cycles: each passes its own checks, the ranks find out together
    shutil.copy(d + "cycle_000003.lgr.0", d + "mixed.lgr.0")
    shutil.copy(d + "cycle_000006.lgr.1", d + "mixed.lgr.1")
    R, _ = run2([["-restart", d + "mixed.lgr"]] * 2)
    assert R == {0: "refused", 1: "refused"}
    assert "pieces of different checkpoints" in capfd.readouterr().err
    # a one-rank restart of the two-rank checkpoint
    shutil.copy(d + "cycle_000003.lgr.0", d + "alone.lgr")
    p = exe(args + ["-restart", d + "alone.lgr"])
    assert p.returncode != 0 and "refused" in p.stderr and "rank 0 of 2" in p.stderr and "step " not in p.stdout
