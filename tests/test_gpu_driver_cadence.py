"""The periodic outputs of the driver (-hist, -prof, -map, -ckpt) on a run whose LAST RK step is a repeated one: the run ends
on the state of the last accepted step with a shortened dt, and each output is due once more for that cycle unless the cycle
has it already - but for the checkpoint, which is written again in any case because dt is part of it.

The run is 1D Sod on 16 zones.  The CPU oracle (oracle.driver.run) takes its RK steps in this sequence, R a repeated and A an
accepted one: R1 R1 R1 R1 A1 R2 A2 A3 A4 R5 A5 ..., and tests/test_gpu_1d.py holds the GPU to the oracle's repeats on this
run.  So `-ms 9` (10 RK steps) ends on the repeat of step 5 with 4 accepted steps and 6 repeats, `-ms 5` (6 RK steps) on the
repeat of step 2 with 1 accepted step and 5 repeats."""
import glob
import os

import numpy as np
import pytest

from test_gpu_history_driver import read_history, strs

pytestmark = pytest.mark.gpu

SOD_1D = ["-p", 2, "-m", "data/segment01.mesh", "-rs", 3]


def run_sim(args):
    from laghos_amd import host_lib
    sim = host_lib.Sim(strs(args) + ["-q"])
    try:
        while True:
            rc = sim.step()
            assert rc >= 0, "a step failed"
            if rc == 0:
                break
        sim.sync()
        return dict(t=sim.t, dt=sim.dt, ti=sim.ti, rk=sim.rk_steps, repeats=sim.repeats, fp=sim.fingerprint(), words=sim.state().size)
    finally:
        sim.close()


def cycles_of(pattern):
    """the cycle numbers in the names of the files that match"""
    return sorted(int(os.path.basename(f).split("_")[-1].split(".")[0]) for f in glob.glob(pattern))


def outputs(base):
    _, rows, _ = read_history(base + "_history.csv")
    return rows, cycles_of(base + "_profile_*.csv"), cycles_of(base + "_map/cycle_*.vti")


def test_run_ends_on_a_repeated_step(tmp_path):
    from laghos_amd import host_lib
    plain = run_sim(SOD_1D + ["-ms", 9, "-k", str(tmp_path / "plain" / "run")])
    assert (plain["rk"], plain["ti"], plain["repeats"]) == (10, 4, 6)
    assert not os.path.exists(str(tmp_path / "plain"))

    # a period that leaves the last accepted step without its output: one more of each
    base = str(tmp_path / "three" / "run")
    A = run_sim(SOD_1D + ["-ms", 9, "-hist", 3, "-prof", 3, "-map", 3, "-ckpt", 3, "-k", base])
    assert (A["rk"], A["ti"], A["repeats"]) == (10, 4, 6)
    rows, prof, maps = outputs(base)
    assert [r["cycle"] for r in rows] == [0, 3, 4]
    assert (rows[-1]["dt"], rows[-1]["rk_steps"], rows[-1]["repeats"]) == (A["dt"], 10, 6)
    assert prof == [0, 3, 4] and maps == [0, 3, 4]
    assert sorted(os.listdir(base + "_restart")) == ["cycle_000003.lgr", "cycle_000004.lgr", "latest"]
    assert open(base + "_restart/latest").read() == "cycle_000004.lgr\n"
    # the outputs leave the run alone
    assert (A["fp"], A["t"], A["dt"]) == (plain["fp"], plain["t"], plain["dt"])

    # a period that has given the last accepted step its output: no second one, but the checkpoint is written again
    base = str(tmp_path / "two" / "run")
    B = run_sim(SOD_1D + ["-ms", 9, "-hist", 2, "-prof", 2, "-map", 2, "-ckpt", 2, "-k", base])
    assert (B["rk"], B["ti"], B["repeats"]) == (10, 4, 6)
    rows, prof, maps = outputs(base)
    assert [r["cycle"] for r in rows] == [0, 2, 4]
    assert prof == [0, 2, 4] and maps == [0, 2, 4]
    assert sorted(os.listdir(base + "_restart")) == ["cycle_000002.lgr", "cycle_000004.lgr", "latest"]   # (-ckpt-keep 2: cycle 4 counts once)
    assert open(base + "_restart/latest").read() == "cycle_000004.lgr\n"
    S, t, c = np.empty(B["words"]), np.empty(4), np.empty(4, dtype=np.int64)
    h = host_lib.host_read_checkpoint(base + "_restart/cycle_000004.lgr", S, t, c)
    assert (h["ti"], h["steps"], h["repeats"]) == (4, 10, 6)
    assert h["dt"] == B["dt"] and rows[-1]["dt"] > B["dt"]     # the shortened dt, not the one the accepted step left

    # the run ends on the repeat of step 2
    base = str(tmp_path / "short" / "run")
    C = run_sim(SOD_1D + ["-ms", 5, "-hist", 3, "-prof", 3, "-map", 3, "-k", base])
    assert (C["rk"], C["ti"], C["repeats"]) == (6, 1, 5)
    rows, prof, maps = outputs(base)
    assert [r["cycle"] for r in rows] == [0, 1] and prof == [0, 1] and maps == [0, 1]
    assert (rows[-1]["dt"], rows[-1]["rk_steps"], rows[-1]["repeats"]) == (C["dt"], 6, 5)
