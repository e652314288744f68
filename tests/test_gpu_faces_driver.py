"""`laghos -pv-surface` / `-pv-slice AXIS K`: the face dumps of the driver through host_lib's sim object and the `laghos`
executable, WITHOUT -paraview - which cycles are written and listed, what the files hold against Sim.face_fields of the same
state (bit for bit), the cells' orientation, one rank against two, a restart, and that nothing changes without the options.

Cycles: `-ms 3 -vs 2` dumps cycles 0, 2 and 4 (tests/test_gpu_paraview_driver.py tells why).

One rank against two (threads on the LGHLOCAL communicator, as tests/test_gpu_restart_driver.py runs them): the pieces of the
two ranks hold, together, the faces the one-rank file holds - keyed by the zone's coordinates in the global grid and the local
face, read off the undeformed points of cycle 0 - and at cycle 0 the same bits for them: the initial state and its density
projection are zone-local.  After steps the two runs differ in the last bits (their solvers sum in another order), so the later
cycles are compared for the faces they hold, and each rank's piece for its bits against that rank's own Sim.face_fields."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

from faces_ref import read_face_vtu, read_pvd
from test_host_faces import BAD, run_refused

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "laghos_amd", "laghos")

RUNS = {
    # id: (mesh options, slice, zones per axis)
    "3D": (["-p", 1, "-m", "data/cube01_hex.mesh", "-rs", 1], ("z", 1), (4, 4, 4)),
    "2D": (["-p", 1, "-m", "data/square01_quad.mesh", "-rs", 1], ("y", 3), (4, 4)),
}
FACE_OPTS = ["-pv-fields", "vorticity,detj"]
CYCLES = [0, 2, 4]


def strs(a):
    return [str(x) for x in a]


def face_args(run, base, on=True):
    mesh, (ax, K), _ = RUNS[run]
    return strs(mesh + ["-ms", 3, "-vs", 2, "-k", base] + (["-pv-surface", "-pv-slice", ax, K] if on else []))


def set_dirs(run, base):
    ax, K = RUNS[run][1]
    return {"surface": base + "_surface", (ax, K): f"{base}_slice_{ax}{K}"}


def check_piece(f, d, dim, R, extras=("vorticity", "detJ")):
    """a face piece `f` (read_face_vtu) against the dict `d` of Sim.face_fields for the same faces: the bits"""
    A = f["arrays"]
    faces = d["faces"]
    NPF, NCF = (R + 1) ** (dim - 1), R ** (dim - 1)
    assert f["npoints"] == len(faces) * NPF and f["ncells"] == len(faces) * NCF          # cell count = face count x cells per face
    assert np.array_equal(f["cell_faces"], np.repeat(faces, NCF, 0))
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    pad = lambda s: np.concatenate([s, np.zeros((3 - dim, s.shape[1]))]).T
    want = {"Points": pad(d["x"]), "velocity": pad(d["v"]), "density": d["rho"], "specific_internal_energy": d["e"], "pressure": d["p"],
            "area_normal": pad(d["area_normal"]), "detJ": d["detj"]}
    vort = np.zeros((len(faces) * NPF, 3))
    if dim == 3:
        vort[:] = d["vorticity"].T
    else:
        vort[:, 2] = d["vorticity"]
    want["vorticity"] = vort
    names = [n for n, s in f["section"].items() if s == "PointData"]
    assert names == ["density", "velocity", "specific_internal_energy", "pressure"] + list(extras) + ["area_normal"]
    for n in ["Points"] + names:
        assert np.array_equal(bits(A[n]), bits(want[n])), n
    # outward-consistent cells: the cell's normal by its corner order agrees with the area vectors at its corners
    if f["ncells"]:
        an = A["area_normal"][f["conn"]].mean(1)
        assert np.all((f["cell_normals"] * an).sum(1) > 0)


@pytest.mark.parametrize("run", list(RUNS))
def test_driver_face_dumps(run, tmp_path):
    from laghos_amd import host_lib
    base = str(tmp_path / "out" / "run")
    (ax, K), zones = RUNS[run][1], RUNS[run][2]
    dim = len(zones)
    sim = host_lib.Sim(face_args(run, base) + strs(FACE_OPTS) + ["-q"])
    try:
        rc = 1
        while rc == 1:
            rc = sim.step()
        assert rc == 0
        sim.sync()
        t_final, sz = sim.t, sim.sizes()
        R = sz["D1D"] - 1                                  # default -vr: order_v
        live = {w: sim.face_fields(R, w) for w in ("surface", (ax, K))}
        with pytest.raises(RuntimeError):
            sim.select_faces((ax, zones["xyz".index(ax)] + 1))
    finally:
        sim.close()
    assert not os.path.exists(base + "_paraview") and not os.path.exists(base + ".pvd")      # no volume dump was asked for
    NE = int(np.prod(zones))
    n_surface = 2 * sum(NE // n for n in zones)
    a = "xyz".index(ax)
    assert len(live["surface"]["faces"]) == n_surface and len(live[(ax, K)]["faces"]) == NE // zones[a]
    assert np.all(live[(ax, K)]["faces"][:, 1] == (2 * a if K < zones[a] else 2 * a + 1))
    for which, d in set_dirs(run, base).items():
        assert sorted(os.listdir(d)) == [f"cycle_{c:06d}.vtu" for c in CYCLES], d
        sets = read_pvd(d + ".pvd")                                                          # the collection lists every dump
        assert [f for _, f in sets] == [f"{os.path.basename(d)}/cycle_{c:06d}.vtu" for c in CYCLES]
        times = [float(t) for t, _ in sets]
        assert times[0] == 0.0 and times[-1] == t_final and all(x < y for x, y in zip(times, times[1:]))
        f = read_face_vtu(f"{d}/cycle_{CYCLES[-1]:06d}.vtu", dim)
        assert f["arrays"]["TIME"][0] == t_final and f["arrays"]["CYCLE"][0] == CYCLES[-1] and np.all(f["arrays"]["rank"] == 0)
        check_piece(f, live[which], dim, R)
        # the slice is the plane it names: at cycle 0 its points have coordinate K / n along the axis
        f0 = read_face_vtu(f"{d}/cycle_000000.vtu", dim)
        if which != "surface":
            assert np.abs(f0["arrays"]["Points"][:, a] - K / zones[a]).max() <= 1e-15
        else:
            on_box = np.isclose(f0["arrays"]["Points"][:, :dim], 0.0, atol=1e-15) | np.isclose(f0["arrays"]["Points"][:, :dim], 1.0, atol=1e-15)
            assert np.all(on_box.any(1))
    assert np.abs(live["surface"]["v"]).max() > 0 and np.abs(live["surface"]["vorticity"]).max() > 0


def test_renumbered_run_selects_the_same_faces(tmp_path):
    """-renumber random: the selection comes from the structured coordinates, so the files hold the same geometry"""
    from laghos_amd import host_lib
    pts = {}
    for name, extra in (("lex", []), ("ren", ["-renumber", "random"])):
        base = str(tmp_path / name / "run")
        sim = host_lib.Sim(strs(RUNS["3D"][0] + ["-ms", 0, "-k", base, "-pv-surface", "-pv-slice", "x", 4, "-q"] + extra))
        sim.close()
        for tag in ("surface", "slice_x4"):
            f = read_face_vtu(f"{base}_{tag}/cycle_000000.vtu", 3)
            P = f["arrays"]["Points"]
            pts[name, tag] = P[np.lexsort(P.T[::-1])]
            assert np.all((f["cell_normals"] * f["arrays"]["area_normal"][f["conn"]].mean(1)).sum(1) > 0)
    for tag in ("surface", "slice_x4"):
        assert np.array_equal(pts["lex", tag], pts["ren", tag]), tag
    assert np.all(pts["ren", "slice_x4"][:, 0] == 1.0) and len(pts["ren", "slice_x4"]) == 16 * 9


# ---- one rank against two ---------------------------------------------------------------------------------------------
def keyed(f, dim, h, f0=None):
    """(zone coordinates in the global grid, local face) -> the PointData of the face, from a piece f; the coordinates are read
    off the undeformed points of the cycle-0 piece f0 of the same faces"""
    f0 = f if f0 is None else f0
    A, P0 = f["arrays"], f0["arrays"]["Points"]
    faces = f["cell_faces"]
    out = {}
    if not len(faces):
        return out
    nfaces = len(np.flatnonzero(np.r_[True, np.any(faces[1:] != faces[:-1], 1)]))
    NPF, NCF = f["npoints"] // nfaces, f["ncells"] // nfaces
    names = [n for n, s in f["section"].items() if s == "PointData"] + ["Points"]
    for k in range(nfaces):
        fc = int(faces[k * NCF, 1])
        a, s = fc >> 1, fc & 1
        c = P0[k * NPF:(k + 1) * NPF, :dim].mean(0) / h
        zc = [int(np.floor(c[b] + 1e-9)) for b in range(dim)]
        zc[a] = int(round(c[a])) - s
        key = (tuple(zc), fc)
        assert key not in out
        out[key] = {n: A[n][k * NPF:(k + 1) * NPF].copy() for n in names}
    return out


def run_ranks(nranks, args, R):
    """every rank's leg in a thread: the sim stepped to its end, then its own face_fields of the final state"""
    from laghos_amd import host_lib
    cid = (b"LGHLOCAL" + os.urandom(16).hex().encode()).ljust(128, b"\0") if nranks > 1 else None
    out, err = {}, {}

    def rank_main(rank):
        try:
            sim = host_lib.Sim(args + ["-q"], nranks=nranks, rank=rank, nccl_id=cid)
            try:
                if nranks > 1:
                    sim.enable_timers(False)
                rc = 1
                while rc == 1:
                    rc = sim.step()
                assert rc == 0
                sim.sync()
                out[rank] = {w: sim.face_fields(R, w) for w in ("surface", ("x", 4), ("z", 2))}
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
    return out


def test_one_rank_against_two(tmp_path):
    dim, R, last = 3, 2, 3
    h = np.array([2 / 8, 1 / 4, 1 / 4])
    mesh = ["-dim", 3, "-nx", 8, "-ny", 4, "-nz", 4, "-Sx", 2, "-Sy", 1, "-Sz", 1, "-rs", 0, "-p", 1, "-ok", 2, "-ot", 1, "-pa", "-tf", 1e9, "-ms", last - 1,
            "-vs", 10 ** 9, "-pv-surface", "-pv-slice", "x", 4, "-pv-slice", "z", 2, "-pv-fields", "vorticity,detj"]
    tags = {"surface": "surface", ("x", 4): "slice_x4", ("z", 2): "slice_z2"}
    union = {}
    for nranks in (1, 2):
        base = str(tmp_path / f"r{nranks}" / "run")
        live = run_ranks(nranks, strs(mesh + ["-k", base]), R)
        for which, tag in tags.items():
            d = f"{base}_{tag}"
            names = [f"cycle_{c:06d}" + (f".{r}" if nranks > 1 else "") + ".vtu" for c in (0, last) for r in range(nranks)]
            assert sorted(os.listdir(d)) == sorted(names + ([f"cycle_{c:06d}.pvtu" for c in (0, last)] if nranks > 1 else []))
            ext = ".pvtu" if nranks > 1 else ".vtu"
            assert [f for _, f in read_pvd(d + ".pvd")] == [f"run_{tag}/cycle_{c:06d}{ext}" for c in (0, last)]
            if nranks > 1:
                txt = open(f"{d}/cycle_{last:06d}.pvtu").read()
                assert re.findall(r'<Piece Source="([^"]+)"/>', txt) == [f"cycle_{last:06d}.{r}.vtu" for r in range(nranks)]
                assert 'Name="area_normal"' in txt and 'Name="face"' in txt and 'Name="vorticity"' in txt
            for c in (0, last):
                merged = {}
                for r in range(nranks):
                    piece = lambda cyc: read_face_vtu(f"{d}/cycle_{cyc:06d}" + (f".{r}" if nranks > 1 else "") + ".vtu", dim)
                    f = piece(c)
                    assert np.all(f["arrays"]["rank"] == r)
                    if c == last:
                        check_piece(f, live[r][which], dim, R)          # each piece: the bits of its own rank's sampling
                    k = keyed(f, dim, h, piece(0))
                    assert not set(k) & set(merged)                      # a face belongs to one rank
                    merged.update(k)
                union[nranks, which, c] = merged
        # the x = 4 plane is the interface of the two ranks: the side-0 faces of layer 4 belong to rank 1 alone, and it is no boundary
        if nranks == 2:
            assert len(live[0][("x", 4)]["faces"]) == 0 and len(live[1][("x", 4)]["faces"]) == 16
            assert read_face_vtu(f"{base}_slice_x4/cycle_000000.0.vtu", dim)["npoints"] == 0     # a rank without faces: an empty piece
            assert len(live[0]["surface"]["faces"]) == len(live[1]["surface"]["faces"]) == 16 + 4 * 16
    for which in tags:
        for c in (0, last):
            one, two = union[1, which, c], union[2, which, c]
            assert set(one) == set(two) and len(one) == {"surface": 2 * (16 + 32 + 32), ("x", 4): 16, ("z", 2): 32}[which], (which, c)
        one, two = union[1, which, 0], union[2, which, 0]
        for key in one:
            for n, a in one[key].items():
                assert np.array_equal(a.view(np.uint64), two[key][n].view(np.uint64)), (which, key, n)


# ---- restart ----------------------------------------------------------------------------------------------------------
def run_to_end(args):
    from laghos_amd import host_lib
    sim = host_lib.Sim(strs(args) + ["-q"])
    try:
        rc = 1
        while rc == 1:
            rc = sim.step()
        assert rc == 0
        sim.sync()
    finally:
        sim.close()


def test_restart_writes_the_same_files(tmp_path):
    base = str(tmp_path / "pv" / "run")
    opts = ["-p", 1, "-m", "data/square01_quad.mesh", "-rs", 1, "-ok", 2, "-ot", 1, "-ms", 6, "-vs", 2, "-pv-surface", "-pv-slice", "x", 2,
            "-pv-fields", "vorticity,detj", "-k", base]
    run_to_end(opts + ["-ckpt", 4, "-ckpt-keep", 0])
    cycles = [0, 2, 4, 6, 7]
    dirs = [base + "_surface", base + "_slice_x2"]
    whole, pvd, stamp = {}, {}, {}
    for d in dirs:
        assert sorted(os.listdir(d)) == [f"cycle_{c:06d}.vtu" for c in cycles]
        whole[d] = {c: open(f"{d}/cycle_{c:06d}.vtu", "rb").read() for c in cycles}
        pvd[d] = open(d + ".pvd").read()
        stamp[d] = os.stat(f"{d}/cycle_000000.vtu").st_mtime_ns
        for c in (6, 7):
            os.remove(f"{d}/cycle_{c:06d}.vtu")
        os.remove(d + ".pvd")
    run_to_end(opts + ["-restart", f"{base}_restart/cycle_000004.lgr"])
    for d in dirs:
        assert open(d + ".pvd").read() == pvd[d]                       # the dumps of both segments, once each, in order
        assert os.stat(f"{d}/cycle_000000.vtu").st_mtime_ns == stamp[d]   # no cycle-0 dump on a restart
        for c in (6, 7):
            assert open(f"{d}/cycle_{c:06d}.vtu", "rb").read() == whole[d][c], (d, c)
    assert not os.path.exists(base + ".pvd")


# ---- without the options ----------------------------------------------------------------------------------------------
def tree(root):
    return sorted(os.path.relpath(os.path.join(dp, f), root) for dp, _, fs in os.walk(root) for f in fs)


def test_without_the_options_nothing_changes(tmp_path):
    """the same 2D run with -paraview -pv-fields, with and without the face options: without them the output has no line of theirs and the
    tree no file of theirs; with them, one line and the new files more - every other line and file is the same to the byte"""
    outs = {}
    timing = re.compile(r"time|rate|FOM|megadofs|ParaView dumps", re.I)
    for name, on in (("base", False), ("again", False), ("faces", True)):
        root = tmp_path / name
        p = subprocess.run([EXE] + face_args("2D", str(root / "run"), on) + strs(FACE_OPTS) + ["-paraview", "-print"], capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert p.returncode == 0, p.stdout + p.stderr
        outs[name] = ([l for l in p.stdout.splitlines() if not timing.search(l)], tree(str(root)), str(root))
    lines, files, root = outs["base"]
    assert (lines, files) == outs["again"][:2] and len(lines) > 8
    assert not any("Face dumps" in l or "_surface" in l or "_slice" in l for l in lines)
    assert not any("_surface" in f or "_slice" in f for f in files)
    lines_f, files_f, root_f = outs["faces"]
    assert [l for l in lines_f if not l.startswith("Face dumps:")] == lines and sum(l.startswith("Face dumps:") for l in lines_f) == 1
    new = [f for f in files_f if f not in files]
    assert sorted(new) == sorted([f"run_{t}/cycle_{c:06d}.vtu" for t in ("surface", "slice_y3") for c in CYCLES] + ["run_surface.pvd", "run_slice_y3.pvd"])
    for f in files:                                                       # the volume dumps and the -print files: the same bytes
        assert open(os.path.join(root, f), "rb").read() == open(os.path.join(root_f, f), "rb").read(), f


@pytest.mark.parametrize("case", list(BAD))
def test_driver_refusals(case, tmp_path):
    run_refused(case, tmp_path)
