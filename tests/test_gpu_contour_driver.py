"""`laghos -pv-iso FIELD VALUE` / `-pv-plane NX NY [NZ] D`: the contour dumps of the driver through host_lib's sim object and the
`laghos` executable, WITHOUT -paraview - which cycles are written and listed, what the files hold against Sim.contour of the same
state (bit for bit), a restart, one rank against two, and that nothing changes without the options.

Cycles: `-ms 6 -vs 3` dumps cycles 0, 3, 6 and 7 (tests/test_gpu_paraview_driver.py tells why the last step is one further).

The density value is found once per run from the final state of a run without outputs: the first of 1 + 1e-2, 1 + 1e-3, ... whose
surface has a few primitives (Sedov starts from rho = 1 and seven steps move it little).

One rank against two (threads on the LGHLOCAL communicator, as tests/test_gpu_faces_driver.py runs them): at cycle 0 the state and
its density projection are zone-local, so the pieces of the two ranks hold, together, the primitives of the one-rank file with the
same bits, zone by zone in the same order - a zone is named by its coordinates in the global grid, read off the centre of its
primitives.  The plane lies in the half of the box that rank 0 holds: rank 1 writes empty pieces."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

from faces_ref import read_pvd
from vtu_reader import read_vtu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "laghos_amd", "laghos")

RUNS = {
    # id: (mesh options, plane numbers)
    "3D": (["-p", 1, "-m", "data/cube01_hex.mesh", "-rs", 1], [1, 0.5, 0.25, 0.8]),
    "2D": (["-p", 1, "-m", "data/square01_quad.mesh", "-rs", 1], [1, 2, 1]),
}
CYCLES = [0, 3, 6, 7]
STEPS = ["-ms", 6, "-vs", 3]


def strs(a):
    return [str(x) for x in a]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def run_sim(args, then=None, **kw):
    from laghos_amd import host_lib
    sim = host_lib.Sim(strs(args) + ["-q"], **kw)
    try:
        rc = 1
        while rc == 1:
            rc = sim.step()
        assert rc == 0
        sim.sync()
        return then(sim) if then else None
    finally:
        sim.close()


_density = {}


def density_value(run):
    """a density value the final state of the run crosses"""
    if run not in _density:
        def find(sim):
            R = sim.sizes()["D1D"] - 1
            for k in range(2, 9):
                if len(sim.contour(R, "density", 1.0 + 10.0 ** -k)["zone"]) >= 8:
                    return 1.0 + 10.0 ** -k
            raise AssertionError("no density value with a surface")
        _density[run] = run_sim(RUNS[run][0] + STEPS + ["-k", "/nonexistent/never/written"], find)
    return _density[run]


def contour_args(run, base, on=True):
    mesh, plane = RUNS[run]
    opts = ["-pv-iso", "density", repr(density_value(run)), "-pv-plane"] + plane + ["-pv-fields", "div_v"] if on else []
    return strs(mesh + STEPS + ["-k", base] + opts)


def check_piece(f, d, dim, iso, rank=0):
    """a contour piece `f` (read_vtu) against the dict `d` of Sim.contour: the bits"""
    A = f["arrays"]
    n = len(d["zone"])
    nv = dim * n
    assert (f["npoints"], f["ncells"]) == (nv, n)
    assert [k for k, s in f["section"].items() if s == "PointData"] == ["density", "velocity", "specific_internal_energy", "pressure", "div_v"]
    assert [k for k, s in f["section"].items() if s == "CellData"] == ["zone", "rank"]
    assert np.all(A["types"] == (5 if dim == 3 else 3)) and np.array_equal(A["offsets"], dim * np.arange(1, n + 1))
    assert np.array_equal(A["connectivity"], np.arange(nv)) and np.array_equal(A["zone"], d["zone"]) and np.all(A["rank"] == rank)
    assert bits(A["ISO_VALUE"])[0] == bits(np.array([float(iso)]))[0]
    pad = lambda s: np.concatenate([s, np.zeros((3 - dim, nv))]).T
    want = {"Points": pad(d["points"]), "velocity": pad(d["v"]), "density": d["rho"], "specific_internal_energy": d["e"], "pressure": d["p"],
            "div_v": d["div_v"]}
    for k, w in want.items():
        assert np.array_equal(bits(A[k]), bits(w)), k


@pytest.mark.parametrize("run", list(RUNS))
def test_driver_contour_dumps(run, tmp_path):
    base = str(tmp_path / "out" / "run")
    plane = RUNS[run][1]
    dim = len(plane) - 1
    rho_iso = density_value(run)

    def live(sim):
        R = sim.sizes()["D1D"] - 1                                  # default -vr: order_v
        out = {"iso0_density": sim.contour(R, "density", rho_iso, fields=("div_v",)),
               "plane0": sim.contour(R, ("plane", plane[:-1], plane[-1]), fields=("div_v",))}
        with pytest.raises(RuntimeError):
            sim.contour(R, "enstrophy", 1.0)
        with pytest.raises(RuntimeError):
            sim.contour(R, "density", float("nan"))
        with pytest.raises(RuntimeError):
            sim.contour(R, ("plane", [0.0] * dim, 1.0))
        return out, sim.t
    got, t_final = run_sim(contour_args(run, base), live)
    assert not os.path.exists(base + "_paraview") and not os.path.exists(base + ".pvd")      # no volume dump was asked for
    for tag, d in got.items():
        directory = f"{base}_{tag}"
        iso = rho_iso if tag.startswith("iso") else plane[-1]
        assert sorted(os.listdir(directory)) == [f"cycle_{c:06d}.vtu" for c in CYCLES], directory
        sets = read_pvd(directory + ".pvd")
        assert [f for _, f in sets] == [f"run_{tag}/cycle_{c:06d}.vtu" for c in CYCLES]
        times = [float(t) for t, _ in sets]
        assert times[0] == 0.0 and times[-1] == t_final and all(x < y for x, y in zip(times, times[1:]))
        f = read_vtu(f"{directory}/cycle_{CYCLES[-1]:06d}.vtu")
        assert f["arrays"]["TIME"][0] == t_final and f["arrays"]["CYCLE"][0] == CYCLES[-1]
        assert len(d["zone"]) >= 8 and d["n_skipped"] == 0
        check_piece(f, d, dim, iso)
    # the plane is the plane it names, and the density surface has the density it names
    P = got["plane0"]["points"]
    assert np.abs(sum(plane[a] * P[a] for a in range(dim)) - plane[-1]).max() <= 1e-14
    assert np.abs(got["iso0_density"]["rho"] - rho_iso).max() <= 1e-14
    # the undeformed plane of cycle 0: its closed-form measure where the whole box is cut (2D: x + 2 y = 1)
    if dim == 2:
        A0 = read_vtu(f"{base}_plane0/cycle_000000.vtu")["arrays"]
        seg = A0["Points"].reshape(-1, 2, 3)
        length = np.linalg.norm(seg[:, 1] - seg[:, 0], axis=1).sum()
        assert abs(length - 0.5 * np.sqrt(5.0)) <= 1e-12 * 0.5 * np.sqrt(5.0)


def test_restart_writes_the_same_files(tmp_path):
    base = str(tmp_path / "pv" / "run")
    opts = contour_args("2D", base)
    run_sim(opts + ["-ckpt", 3, "-ckpt-keep", 0])
    dirs = [base + "_iso0_density", base + "_plane0"]
    whole, pvd, stamp = {}, {}, {}
    for d in dirs:
        assert sorted(os.listdir(d)) == [f"cycle_{c:06d}.vtu" for c in CYCLES]
        whole[d] = {c: open(f"{d}/cycle_{c:06d}.vtu", "rb").read() for c in CYCLES}
        pvd[d] = open(d + ".pvd").read()
        stamp[d] = os.stat(f"{d}/cycle_000000.vtu").st_mtime_ns
        for c in (6, 7):
            os.remove(f"{d}/cycle_{c:06d}.vtu")
        os.remove(d + ".pvd")
    run_sim(opts + ["-restart", f"{base}_restart/cycle_000003.lgr"])
    for d in dirs:
        assert open(d + ".pvd").read() == pvd[d]                          # the dumps of both segments, once each, in order
        assert os.stat(f"{d}/cycle_000000.vtu").st_mtime_ns == stamp[d]   # no cycle-0 dump on a restart
        for c in (6, 7):
            assert open(f"{d}/cycle_{c:06d}.vtu", "rb").read() == whole[d][c], (d, c)
    assert not os.path.exists(base + ".pvd")


def tree(root):
    return sorted(os.path.relpath(os.path.join(dp, f), root) for dp, _, fs in os.walk(root) for f in fs)


def test_without_the_options_nothing_changes(tmp_path):
    """the same 2D run with -paraview -pv-fields, with and without the two options: without them the output has no line of theirs
    and the tree no file of theirs; with them, one line and the new files more - every other line and file is the same to the byte"""
    outs = {}
    timing = re.compile(r"time|rate|FOM|megadofs|ParaView dumps", re.I)
    for name, on in (("base", False), ("again", False), ("contours", True)):
        root = tmp_path / name
        args = contour_args("2D", str(root / "run"), on) + ([] if on else ["-pv-fields", "div_v"]) + ["-paraview", "-print"]
        p = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert p.returncode == 0, p.stdout + p.stderr
        outs[name] = ([l for l in p.stdout.splitlines() if not timing.search(l)], tree(str(root)), str(root))
    lines, files, root = outs["base"]
    assert (lines, files) == outs["again"][:2] and len(lines) > 8
    assert not any("Contour dumps" in l or "_iso" in l or "_plane" in l for l in lines)
    assert not any("_iso" in f or "_plane" in f for f in files)
    assert [f for f in files if f.startswith("run_paraview/")] == [f"run_paraview/cycle_{c:06d}.vtu" for c in CYCLES]   # written when -paraview writes
    lines_c, files_c, root_c = outs["contours"]
    assert [l for l in lines_c if not l.startswith("Contour dumps:")] == lines and sum(l.startswith("Contour dumps:") for l in lines_c) == 1
    new = [f for f in files_c if f not in files]
    assert sorted(new) == sorted([f"run_{t}/cycle_{c:06d}.vtu" for t in ("iso0_density", "plane0") for c in CYCLES] + ["run_iso0_density.pvd", "run_plane0.pvd"])
    for f in files:                                                       # the volume dumps and the -print files: the same bytes
        assert open(os.path.join(root, f), "rb").read() == open(os.path.join(root_c, f), "rb").read(), f


# ---- one rank against two ---------------------------------------------------------------------------------------------
PLANE_2R = [1, 0.3, 0.2, 0.4567]    # inside x < 1, the half of the 2 x 1 x 1 box that rank 0 holds; through no lattice point


def run_ranks(nranks, args, R):
    """every rank's leg in a thread: the sim stepped to its end, then its own contour of the final state"""
    cid = (b"LGHLOCAL" + os.urandom(16).hex().encode()).ljust(128, b"\0") if nranks > 1 else None
    out, err = {}, {}

    def rank_main(rank):
        try:
            def live(sim):
                if nranks > 1:
                    sim.enable_timers(False)
                return sim.contour(R, ("plane", PLANE_2R[:3], PLANE_2R[3]), fields=("div_v",))
            out[rank] = run_sim(args, live, nranks=nranks, rank=rank, nccl_id=cid)
        except Exception as ex:  # noqa: BLE001 - reported below
            err[rank] = repr(ex)

    th = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(nranks)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in th) and not err, err
    return out


def by_zone(f, h):
    """zone coordinates in the global grid -> the points of its primitives, in the file's order"""
    P = f["arrays"]["Points"].reshape(-1, 3, 3)
    out = {}
    for tri in P:
        key = tuple(int(c) for c in np.floor(tri.mean(0) / h))
        out.setdefault(key, []).append(tri)
    return {k: np.array(v) for k, v in out.items()}


def test_one_rank_against_two(tmp_path):
    dim, R, last = 3, 2, 3
    h = np.array([2 / 8, 1 / 4, 1 / 4])
    mesh = ["-dim", 3, "-nx", 8, "-ny", 4, "-nz", 4, "-Sx", 2, "-Sy", 1, "-Sz", 1, "-rs", 0, "-p", 1, "-ok", 2, "-ot", 1, "-pa", "-tf", 1e9, "-ms", last - 1,
            "-vs", 10 ** 9, "-pv-plane"] + PLANE_2R + ["-pv-fields", "div_v"]
    zones = {}
    for nranks in (1, 2):
        base = str(tmp_path / f"r{nranks}" / "run")
        live = run_ranks(nranks, mesh + ["-k", base], R)
        d = f"{base}_plane0"
        names = [f"cycle_{c:06d}" + (f".{r}" if nranks > 1 else "") + ".vtu" for c in (0, last) for r in range(nranks)]
        assert sorted(os.listdir(d)) == sorted(names + ([f"cycle_{c:06d}.pvtu" for c in (0, last)] if nranks > 1 else []))
        ext = ".pvtu" if nranks > 1 else ".vtu"
        assert [f for _, f in read_pvd(d + ".pvd")] == [f"run_plane0/cycle_{c:06d}{ext}" for c in (0, last)]
        if nranks > 1:
            txt = open(f"{d}/cycle_{last:06d}.pvtu").read()
            assert re.findall(r'<Piece Source="([^"]+)"/>', txt) == [f"cycle_{last:06d}.{r}.vtu" for r in range(nranks)]
            assert 'Name="div_v"' in txt and 'Name="zone"' in txt and 'Name="area_normal"' not in txt
        merged = {}
        for r in range(nranks):
            piece = lambda c: read_vtu(f"{d}/cycle_{c:06d}" + (f".{r}" if nranks > 1 else "") + ".vtu")
            check_piece(piece(last), live[r], dim, PLANE_2R[3], rank=r)       # each piece: the bits of its own rank's contour
            k = by_zone(piece(0), h)
            assert not set(k) & set(merged)                                   # a zone belongs to one rank
            merged.update(k)
        zones[nranks] = merged
        if nranks == 2:
            assert len(live[0]["zone"]) > 0 and len(live[1]["zone"]) == 0
            for c in (0, last):
                empty = read_vtu(f"{d}/cycle_{c:06d}.1.vtu")                  # the rank the plane misses: an empty piece
                assert (empty["npoints"], empty["ncells"]) == (0, 0)
    one, two = zones[1], zones[2]
    assert set(one) == set(two) and len(one) > 4
    for key in one:
        assert one[key].shape == two[key].shape and np.array_equal(bits(one[key]), bits(two[key])), key
