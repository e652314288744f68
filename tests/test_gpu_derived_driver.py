"""`laghos -paraview -pv-fields LIST`: the derived fields in the dumps of the driver - which arrays a file holds and in
which order, their content against Sim.derived_fields and the numpy reference (tests/derived_ref.py) of the state, a
subset, two ranks, a restart, and the files without the option."""
import os
import re
import threading

import numpy as np
import pytest

from derived_ref import TOL, derived_reference, lattice_tables3
from vtu_reader import read_vtu

pytestmark = pytest.mark.gpu

STANDING = ["density", "velocity", "specific_internal_energy", "pressure"]
DERIVED = ["div_v", "vorticity", "velocity_gradient", "detJ", "sound_speed"]
NCOMP = dict(div_v=1, vorticity=3, velocity_gradient=9, detJ=1, sound_speed=1)


def strs(a):
    return [str(x) for x in a]


def run_sim(args, nranks=1, rank=0, cid=None, at_end=None):
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
        return at_end(sim) if at_end else sim.ti
    finally:
        sim.close()


def point_arrays(f):
    return [n for n, s in f["section"].items() if s == "PointData"]


def test_taylor_green_2d_all_fields(tmp_path):
    from laghos_amd import host_lib
    base = str(tmp_path / "tg" / "run")
    ok, ot, R = 2, 1, 2
    args = ["-p", 0, "-m", "data/square01_quad.mesh", "-rs", 1, "-ok", ok, "-ot", ot, "-ms", 3, "-vs", 2, "-paraview", "-pv-fields", "all",
            "-k", base]
    # stepped by hand: the state and Sim.derived_fields are taken right after the step that wrote a dump (a repeated step
    # counts towards -ms, so the last dump need not be the last thing the run does)
    sim = host_lib.Sim(strs(args) + ["-q"])
    try:
        sz, seen, rc = sim.sizes(), {}, 1
        while rc == 1:
            rc = sim.step()
            assert rc >= 0, "a step failed"
            if sim.ti not in seen and os.path.exists(f"{base}_paraview/cycle_{sim.ti:06d}.vtu"):
                sim.sync()
                seen[sim.ti] = (sim.state(), sim.derived_fields(R))
    finally:
        sim.close()
    dim, NE = sz["dim"], sz["NE"]
    cycles = sorted(int(re.search(r"cycle_(\d{6})\.vtu$", n).group(1)) for n in os.listdir(base + "_paraview"))
    print(f"dumps at cycles {cycles}")
    assert cycles[0] == 0 and len(cycles) >= 2 and cycles[1:] == sorted(seen)
    ti = cycles[-1]
    S, own = seen[ti]
    files = {c: read_vtu(f"{base}_paraview/cycle_{c:06d}.vtu") for c in cycles}
    for c, f in files.items():
        assert point_arrays(f) == STANDING + DERIVED, c               # every dump, in the table's order
        for n in DERIVED:
            assert f["ncomp"][n] == NCOMP[n] and f["types"][n] == "Float64" and np.isfinite(f["arrays"][n]).all(), (c, n)
    # the last file against Sim.derived_fields of the final state: the same kernel on the same state, the same bits
    a = files[ti]["arrays"]
    NP = files[ti]["npoints"]
    assert NP == NE * (R + 1) ** dim and set(own) == {"detj", "grad_v", "div_v", "vorticity", "sound_speed"}
    assert np.array_equal(a["div_v"], own["div_v"]) and np.array_equal(a["detJ"], own["detj"])
    assert np.array_equal(a["sound_speed"], own["sound_speed"])
    assert np.array_equal(a["vorticity"][:, 2], own["vorticity"]) and not a["vorticity"][:, :2].any()   # the 2D scalar sits in z
    G = a["velocity_gradient"].reshape(NP, 3, 3)
    assert np.array_equal(G[:, :2, :2].reshape(NP, 4).T, own["grad_v"])                                 # row-major 3 i + j
    assert not G[:, 2, :].any() and not G[:, :, 2].any()                                                # zeros beyond dim
    # ... and against the numpy reference of Sim.state()
    d = host_lib.host_disc("square01_quad", 1, ok, ot, 0)
    N = int(d["h1map"].max()) + 1
    ref = derived_reference(dim, NE, N, ok + 1, ot + 1, d["h1map"], S, d["gamma"], *lattice_tables3(ok, ot, R))
    errL = np.sqrt(((own["grad_v"] - ref["grad_v"]) ** 2).sum(0))
    errD = np.abs(own["detj"] - ref["detj"])
    print(f"grad_v: max err / bound {np.max(errL / (TOL * ref['bound_L'])):.4f}; detJ: {np.max(errD / (TOL * ref['bound_det'])):.4f}")
    assert np.all(errL <= TOL * ref["bound_L"]) and np.all(errD <= TOL * ref["bound_det"])
    assert np.all(np.abs(own["sound_speed"] - ref["sound_speed"]) <= 1e-13 * np.abs(ref["sound_speed"]).max()) and ref["e"].min() > 0
    # cycle 0: the velocity is the interpolant of a divergence-free field
    a0 = files[0]["arrays"]
    ratio = np.abs(a0["div_v"]).max() / np.abs(a0["vorticity"]).max()
    print(f"cycle 0: max|div v| / max|vorticity| = {ratio:.3e}")
    assert ratio < 1


def test_sedov_3d_with_a_subset(tmp_path):
    base = str(tmp_path / "sedov" / "run")
    args = ["-p", 1, "-m", "data/cube01_hex.mesh", "-rs", 1, "-ok", 2, "-ot", 1, "-ms", 4, "-vs", 2, "-paraview", "-pv-fields", "detj,div_v",
            "-k", base]
    ti = run_sim(args)
    for c in (0, 2, 4, ti):
        f = read_vtu(f"{base}_paraview/cycle_{c:06d}.vtu")
        assert point_arrays(f) == STANDING + ["div_v", "detJ"], c     # the table's order, whatever order the option gave
    a = f["arrays"]
    print(f"cycle {ti}: div v in [{a['div_v'].min():.3e}, {a['div_v'].max():.3e}], min detJ {a['detJ'].min():.3e}")
    assert a["div_v"].min() < 0


def test_all_in_1d_leaves_the_vorticity_out(tmp_path):
    base = str(tmp_path / "sod" / "run")
    ti = run_sim(["-p", 2, "-m", "data/segment01.mesh", "-rs", 3, "-ms", 30, "-vs", 10, "-paraview", "-pv-fields", "all", "-k", base])
    f = read_vtu(f"{base}_paraview/cycle_{ti:06d}.vtu")
    assert point_arrays(f) == STANDING + ["div_v", "velocity_gradient", "detJ", "sound_speed"]
    a = f["arrays"]
    assert np.array_equal(a["velocity_gradient"][:, 0], a["div_v"]) and not a["velocity_gradient"][:, 1:].any()   # dv/dx alone
    assert a["detJ"].min() > 0 and a["div_v"].min() < 0 and a["sound_speed"].min() > 0


def test_without_pv_fields_the_standing_arrays_alone(tmp_path):
    base = str(tmp_path / "plain" / "run")
    ti = run_sim(["-p", 1, "-m", "data/square01_quad.mesh", "-rs", 1, "-ok", 2, "-ot", 1, "-ms", 2, "-vs", 2, "-paraview", "-k", base])
    for c in (0, ti):
        assert point_arrays(read_vtu(f"{base}_paraview/cycle_{c:06d}.vtu")) == STANDING


def test_restart_writes_the_same_files(tmp_path):
    base = str(tmp_path / "pv" / "run")
    opts = ["-p", 1, "-m", "data/square01_quad.mesh", "-rs", 1, "-ok", 2, "-ot", 1, "-ms", 6, "-vs", 2, "-paraview", "-pv-fields", "all", "-k", base]
    run_sim(opts + ["-ckpt", 4, "-ckpt-keep", 0])
    cycles = [0, 2, 4, 6, 7]
    whole = {c: open(f"{base}_paraview/cycle_{c:06d}.vtu", "rb").read() for c in cycles}
    assert point_arrays(read_vtu(f"{base}_paraview/cycle_000007.vtu")) == STANDING + DERIVED
    for c in (6, 7):
        os.remove(f"{base}_paraview/cycle_{c:06d}.vtu")
    run_sim(opts + ["-restart", f"{base}_restart/cycle_000004.lgr"])
    for c in (6, 7):
        assert open(f"{base}_paraview/cycle_{c:06d}.vtu", "rb").read() == whole[c], c


def test_two_ranks(tmp_path):
    """two 2D blocks of 4 x 4 zones as threads in one process (the LGHLOCAL communicator, as tests/test_gpu_restart_driver.py)"""
    base = str(tmp_path / "two" / "run")
    args = ["-dim", 2, "-nx", 8, "-ny", 4, "-Sx", 2, "-Sy", 1, "-rs", 0, "-p", 1, "-ok", 2, "-ot", 1, "-pa", "-tf", 1e9, "-ms", 2, "-vs", 10 ** 9,
            "-paraview", "-pv-fields", "vorticity,div_v,sound_speed", "-k", base]
    cid = (b"LGHLOCAL" + os.urandom(16).hex().encode()).ljust(128, b"\0")
    out, err = {}, {}

    def rank_main(rank):
        try:
            out[rank] = run_sim(args, nranks=2, rank=rank, cid=cid)
        except Exception as ex:  # noqa: BLE001 - reported below
            err[rank] = repr(ex)

    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in th) and not err, err
    ti = out[0]
    want = ["div_v", "vorticity", "sound_speed"]
    for c in (0, ti):
        for r in range(2):
            f = read_vtu(f"{base}_paraview/cycle_{c:06d}.{r}.vtu")
            assert point_arrays(f) == STANDING + want and all(np.isfinite(f["arrays"][n]).all() for n in want)
            assert np.all(f["arrays"]["rank"] == r)
        txt = open(f"{base}_paraview/cycle_{c:06d}.pvtu").read()
        ppd = re.search(r"<PPointData.*?</PPointData>", txt, flags=re.S).group(0)
        got = re.findall(r'<PDataArray type="Float64" Name="([^"]+)" NumberOfComponents="(\d+)"/>', ppd)
        assert got == [("density", "1"), ("velocity", "3"), ("specific_internal_energy", "1"), ("pressure", "1")] + [(n, str(NCOMP[n])) for n in want]
    # after the steps the blast has moved the fluid: the two pieces hold a flow
    last = [read_vtu(f"{base}_paraview/cycle_{ti:06d}.{r}.vtu")["arrays"] for r in range(2)]
    assert max(np.abs(a["div_v"]).max() for a in last) > 0
