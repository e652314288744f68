"""`laghos -paraview`: the dumps of the driver through host_lib's sim object and the `laghos` executable - which cycles are
written, the collection, and the content of the last file against a numpy evaluation of the final state
(tests/lattice_ref.py) and of the density dofs the `-print` files of the same step hold.

`-ms N` ends the run as the reference's time loop does (laghos.cpp:742-760: the step that finds steps == max_tsteps is
still taken), so `-ms 3 -vs 2` dumps cycles 0, 2 and 4, `-ms 2 -vs 2` cycles 0, 2 and 3: cycle 0, every second step, the
last step - the cycles `-print` writes, plus cycle 0.  A repeated step (dt * 0.85, laghos.cpp:762-778) counts towards -ms
as it does there: the 1D Sod run `-rs 3 -ms 2` repeats its first step three times and ends without an accepted one (cycle 0
alone, `-print` writes nothing), so the 1D case runs the same mesh and problem with `-ms 30`, which gets past the repeats."""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from lattice_ref import lattice_tables, sample_reference
from vtu_reader import read_vtu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "laghos_amd", "laghos")

RUNS = {
    # id: (mesh, rs, problem, options, R, cycles expected)
    "2D": ("square01_quad", 1, 1, ["-ms", 3], 2, [0, 2, 4]),
    "3D": ("cube01_hex", 1, 1, ["-ms", 2, "-vr", 2], 2, [0, 2, 3]),
    "1D": ("segment01", 3, 2, ["-ms", 30], 2, list(range(0, 25, 2)) + [25]),   # (31 steps taken, 6 of them repeated)
}


def run_args(run, base, paraview=True, quiet=True):
    mesh, rs, problem, extra, _, _ = RUNS[run]
    a = ["-p", problem, "-m", f"data/{mesh}.mesh", "-rs", rs] + extra + ["-vs", 2] + (["-paraview"] if paraview else [])
    return [str(x) for x in a + ["-print", "-k", base] + (["-q"] if quiet else [])]


def dumped_cycles(base):
    return sorted(int(re.search(r"cycle_(\d{6})\.vtu$", f).group(1)) for f in glob.glob(base + "_paraview/cycle_*.vtu"))


@pytest.mark.parametrize("run", list(RUNS))
def test_driver_dumps(run, tmp_path):
    from laghos_amd import host_lib
    mesh, rs, problem, _, R, want_cycles = RUNS[run]
    base = str(tmp_path / "out" / "run")
    sim = host_lib.Sim(run_args(run, base))
    try:
        rc = 1
        while rc == 1:
            rc = sim.step()
        assert rc == 0                                # (-1: a crashed time step or a write failure)
        sim.sync()
        t_final, ti, S, sz = sim.t, sim.ti, sim.state(), sim.sizes()
    finally:
        sim.close()
    dim, NE, D, L = sz["dim"], sz["NE"], sz["D1D"], sz["L1D"]
    ok, ot = D - 1, L - 1
    assert R == ok or "-vr" in RUNS[run][3]          # default: order_v cells per zone and direction
    # which cycles: 0, every second step, the last one - those `-print` wrote, and cycle 0; nothing else in the directory
    printed = sorted(int(re.search(r"_(\d+)_rho$", f).group(1)) for f in glob.glob(base + "_*_rho"))
    cycles = dumped_cycles(base)
    print(f"{run}: dumps at cycles {cycles}, -print at {printed}, {ti} accepted steps, t = {t_final}")
    assert cycles == [0] + printed and cycles[-1] == ti
    assert cycles == want_cycles and ti > 0
    assert sorted(os.listdir(base + "_paraview")) == [f"cycle_{c:06d}.vtu" for c in cycles]
    # the collection
    txt = open(base + ".pvd").read()
    sets = re.findall(r'<DataSet timestep="([^"]+)"[^>]* file="([^"]+)"', txt)
    assert [f for _, f in sets] == [f"run_paraview/cycle_{c:06d}.vtu" for c in cycles]
    times = [float(t) for t, _ in sets]
    assert len(times) == len(cycles) and times[0] == 0.0 and times[-1] == t_final
    assert all(a < b for a, b in zip(times, times[1:]))
    # the last file against the final state
    d = host_lib.host_disc(mesh, rs, ok, ot, problem)
    N = int(d["h1map"].max()) + 1
    assert S.size == 2 * dim * N + NE * L ** dim
    rho_dofs = np.loadtxt(f"{base}_{ti}_rho", skiprows=5)   # 8 significant digits
    assert rho_dofs.size == NE * L ** dim
    Bh, Bl = lattice_tables(ok, ot, R)
    ref = sample_reference(dim, NE, N, D, L, d["h1map"], S, rho_dofs, d["gamma"], Bh, Bl)
    f = read_vtu(f"{base}_paraview/cycle_{ti:06d}.vtu")
    a = f["arrays"]
    NPZ = (R + 1) ** dim
    assert f["npoints"] == NE * NPZ and f["ncells"] == NE * R ** dim
    assert a["TIME"][0] == t_final and a["CYCLE"][0] == ti
    pad = lambda s: np.concatenate([s, np.zeros((3 - dim, s.shape[1]))]).T
    for name, want in (("Points", pad(ref["x"])), ("velocity", pad(ref["v"])), ("specific_internal_energy", ref["e"])):
        err, scale = np.abs(a[name] - want).max(), np.abs(want).max()
        print(f"{run} {name}: max err {err:.3e}, max {scale:.3e}")
        assert err <= 1e-13 * scale, (name, err, scale)
    err, scale = np.abs(a["density"] - ref["rho"]).max(), np.abs(ref["rho"]).max()
    print(f"{run} density vs the -print dofs: max err {err:.3e}, max {scale:.3e}")
    assert err <= 1e-7 * scale
    gamma_pt = np.repeat(d["gamma"], NPZ)
    p_own = (gamma_pt - 1.0) * a["density"] * np.maximum(a["specific_internal_energy"], 0.0)
    assert np.abs(a["pressure"] - p_own).max() <= 1e-14 * np.abs(p_own).max()
    assert np.abs(p_own).max() > 0 and np.all(a["rank"] == 0)
    assert np.array_equal(a["zone"], np.repeat(np.arange(NE), R ** dim))
    # the first file holds the initial state
    a0 = read_vtu(f"{base}_paraview/cycle_000000.vtu")["arrays"]
    ref0 = sample_reference(dim, NE, N, D, L, d["h1map"], d["S0"], d["rho0_l2"], d["gamma"], Bh, Bl)
    assert a0["TIME"][0] == 0.0 and a0["CYCLE"][0] == 0
    assert np.abs(a0["Points"] - pad(ref0["x"])).max() <= 1e-13 * np.abs(ref0["x"]).max()


def step_lines(out):
    return [l for l in out.splitlines() if l.startswith("step ")]


def test_without_paraview_nothing_changes(tmp_path):
    """the same 2D run with and without -paraview: no directory and no collection without it, and the same `step` lines"""
    outs = {}
    for name, on in (("with", True), ("without", False)):
        base = str(tmp_path / name / "run")
        p = subprocess.run([EXE] + run_args("2D", base, paraview=on, quiet=False), capture_output=True, text=True, timeout=300,
                           cwd=ROOT)
        assert p.returncode == 0, p.stdout + p.stderr
        outs[name] = (base, p.stdout)
    base, out = outs["without"]
    assert not os.path.exists(base + "_paraview") and not os.path.exists(base + ".pvd")
    assert glob.glob(base + "_*_rho")                       # (-print still writes its files)
    assert "ParaView" not in out
    base_w, out_w = outs["with"]
    assert dumped_cycles(base_w) == RUNS["2D"][5] and os.path.exists(base_w + ".pvd")
    assert len(step_lines(out)) == 2 and step_lines(out) == step_lines(out_w)
    strip = lambda o: [l for l in o.splitlines() if not l.startswith("ParaView dumps:")]
    assert len(strip(out)) == len(strip(out_w))             # one line more with -paraview, nothing else


@pytest.mark.parametrize("vr", [0, 9])
def test_vis_refine_out_of_range_is_refused_before_the_gpu(vr, tmp_path):
    base = str(tmp_path / "run")
    p = subprocess.run([EXE] + run_args("2D", base) + ["-vr", str(vr)], capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert p.returncode != 0 and "-vr" in p.stderr and str(vr) in p.stderr
    assert not glob.glob(str(tmp_path / "*"))               # nothing was set up, nothing written
