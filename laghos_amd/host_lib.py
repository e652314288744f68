"""ctypes binding of liblaghos_host.so: the C++ host layer (reference API mirror,
driver, time loop).  bench.py and the end-to-end tests drive it through these
entry points; numerics run in liblaghos_hip.so."""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblaghos_host.so")
_lib = None


def _preload_torch_hip():
    """torch bundles its own libamdhip64; if this library pulled in /opt/rocm's copy
    first, a later `import torch` would bring a second HIP runtime into the process
    and fail with "No HIP GPUs are available".  Importing torch first makes both
    share one runtime (the standalone `laghos` executable does not involve torch)."""
    try:
        import torch  # noqa: F401
    except Exception:
        pass


def load():
    global _lib
    if _lib is None:
        _preload_torch_hip()
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run __graft_entry__.build()")
        L = ctypes.CDLL(LIB_PATH)
        P, I, D, Lg = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_long
        L.laghos_sim_create.restype = P
        L.laghos_sim_create.argtypes = [I, ctypes.POINTER(ctypes.c_char_p), I, I, ctypes.c_char_p]
        L.laghos_sim_destroy.argtypes = [P]
        L.laghos_sim_step.restype = I
        L.laghos_sim_step.argtypes = [P]
        for n in ("laghos_sim_time", "laghos_sim_dt", "laghos_sim_enorm", "laghos_sim_energy", "laghos_sim_sedov_error"):
            getattr(L, n).restype = D
            getattr(L, n).argtypes = [P]
        for n in ("laghos_sim_steps", "laghos_sim_ti"):
            getattr(L, n).restype = I
            getattr(L, n).argtypes = [P]
        L.laghos_sim_sync.argtypes = [P]
        L.laghos_sim_enable_timers.argtypes = [P, I]
        L.laghos_sim_reset_timers.argtypes = [P]
        L.laghos_sim_timers.argtypes = [P, ctypes.POINTER(D), ctypes.POINTER(Lg)]
        L.laghos_sim_sizes.argtypes = [P, ctypes.POINTER(Lg)]
        L.laghos_sim_context.restype = P
        L.laghos_sim_context.argtypes = [P]
        L.laghos_sim_state_size.restype = Lg
        L.laghos_sim_state_size.argtypes = [P]
        L.laghos_sim_get_state.argtypes = [P, P]
        L.laghos_main.restype = I
        L.laghos_main.argtypes = [I, ctypes.POINTER(ctypes.c_char_p)]
        L.laghos_host_partition.restype = I
        L.laghos_host_partition.argtypes = [I, I, I, I, I, ctypes.POINTER(I)]
        L.laghos_host_tables.restype = I
        L.laghos_host_tables.argtypes = [I, I, P, P, P, P, P, P]
        L.laghos_host_lattice_tables.restype = I
        L.laghos_host_lattice_tables.argtypes = [I, I, I, P, P]
        L.laghos_host_write_vtu.restype = I
        L.laghos_host_write_vtu.argtypes = [ctypes.c_char_p, I, I, I, P, P, P, P, P, I, D, I, I]
        L.laghos_host_write_pvtu.restype = I
        L.laghos_host_write_pvtu.argtypes = [ctypes.c_char_p, I, D, I]
        L.laghos_host_write_pvd.restype = I
        L.laghos_host_write_pvd.argtypes = [ctypes.c_char_p, ctypes.c_char_p, I, P, P, I]
        L.laghos_host_lattice_grad_table.restype = I
        L.laghos_host_lattice_grad_table.argtypes = [I, I, P]
        L.laghos_host_write_vtu_fields.restype = I
        L.laghos_host_write_vtu_fields.argtypes = [ctypes.c_char_p, I, I, I, P, P, P, P, P, I, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(I),
                                                   ctypes.POINTER(P), I, D, I, I]
        L.laghos_host_write_pvtu_fields.restype = I
        L.laghos_host_write_pvtu_fields.argtypes = [ctypes.c_char_p, I, D, I, I, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(I)]
        L.laghos_host_write_vtu_faces.restype = I
        L.laghos_host_write_vtu_faces.argtypes = [ctypes.c_char_p, I, I, P, I, P, P, P, P, P, I, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(I),
                                                  ctypes.POINTER(P), P, I, D, I, I]
        L.laghos_host_write_pvtu_faces.restype = I
        L.laghos_host_write_pvtu_faces.argtypes = [ctypes.c_char_p, I, D, I, I, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(I)]
        L.laghos_sim_select_faces.restype = I
        L.laghos_sim_select_faces.argtypes = [P, I, I, I, P]
        L.laghos_sim_face_fields.restype = I
        L.laghos_sim_face_fields.argtypes = [P, I, I, P, P]
        L.laghos_host_write_vtu_contour.restype = I
        L.laghos_host_write_vtu_contour.argtypes = [ctypes.c_char_p, I, Lg, P, P, P, P, P, P, I, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(I),
                                                    ctypes.POINTER(P), D, I, D, I, I]
        L.laghos_host_write_pvtu_contour.restype = I
        L.laghos_host_write_pvtu_contour.argtypes = [ctypes.c_char_p, I, D, I, I, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(I)]
        L.laghos_sim_contour.restype = Lg
        L.laghos_sim_contour.argtypes = [P, I, ctypes.c_char_p, P, D, ctypes.c_uint, ctypes.POINTER(Lg)]
        L.laghos_sim_contour_get.restype = I
        L.laghos_sim_contour_get.argtypes = [P, P, P]
        L.laghos_sim_derived_fields.restype = I
        L.laghos_sim_derived_fields.argtypes = [P, I, P, P, P, P, P]
        ULL = ctypes.c_ulonglong
        L.laghos_sim_repeats.restype = I
        L.laghos_sim_repeats.argtypes = [P]
        L.laghos_sim_checks.argtypes = [P, ctypes.POINTER(I)]
        L.laghos_sim_error.restype = ctypes.c_char_p
        L.laghos_sim_error.argtypes = [P]
        L.laghos_sim_fingerprint.restype = I
        L.laghos_sim_fingerprint.argtypes = [P, ctypes.POINTER(ULL)]
        L.laghos_sim_write_checkpoint.restype = I
        L.laghos_sim_write_checkpoint.argtypes = [P, ctypes.c_char_p]
        L.laghos_host_write_checkpoint.restype = I
        L.laghos_host_write_checkpoint.argtypes = [ctypes.c_char_p, P, P, P, P, Lg, P, P, Lg, ctypes.c_char_p, I]
        L.laghos_host_read_checkpoint.restype = I
        L.laghos_host_read_checkpoint.argtypes = [ctypes.c_char_p, P, P, P, P, Lg, P, P, Lg, ctypes.c_char_p, I]
        L.laghos_sim_records.restype = Lg
        L.laghos_sim_records.argtypes = [P, ctypes.c_char_p, P, ctypes.POINTER(D)]
        L.laghos_host_write_records_sidecar.restype = I
        L.laghos_host_write_records_sidecar.argtypes = [ctypes.c_char_p, P, Lg, D, I, I, D, I, ctypes.c_char_p, P, P, ctypes.c_char_p, I]
        L.laghos_host_read_records_sidecar.restype = I
        L.laghos_host_read_records_sidecar.argtypes = [ctypes.c_char_p, P, P, P, ctypes.c_char_p, I, P, I, P, Lg, ctypes.c_char_p, I]
        L.laghos_host_match_records_sidecar.restype = I
        L.laghos_host_match_records_sidecar.argtypes = [ctypes.c_char_p, P, I, I, D, I, ctypes.c_char_p, P, ctypes.c_char_p, I]
        L.laghos_sim_diagnostics.argtypes = [P, P]
        L.laghos_sim_profile.restype = I
        L.laghos_sim_profile.argtypes = [P, I, I, D, D, P, P, ctypes.POINTER(Lg)]
        L.laghos_sim_map.restype = I
        L.laghos_sim_map.argtypes = [P, P, P, P, P, ctypes.POINTER(Lg)]
        L.laghos_sim_loads.restype = I
        L.laghos_sim_loads.argtypes = [P, I, P, P, ctypes.POINTER(Lg)]
        L.laghos_host_loads_header.restype = ctypes.c_char_p
        L.laghos_host_loads_header.argtypes = []
        L.laghos_host_loads_text.restype = I
        L.laghos_host_loads_text.argtypes = [Lg, D, ctypes.c_char_p, P, ctypes.c_char_p, I]
        L.laghos_host_loads_write.restype = I
        L.laghos_host_loads_write.argtypes = [ctypes.c_char_p, Lg, ctypes.c_char_p, ctypes.POINTER(Lg), ctypes.c_char_p, I]
        L.laghos_sim_gauges.restype = I
        L.laghos_sim_gauges.argtypes = [P, I, P, P]
        L.laghos_host_gauges_header.restype = ctypes.c_char_p
        L.laghos_host_gauges_header.argtypes = []
        L.laghos_host_gauges_text.restype = I
        L.laghos_host_gauges_text.argtypes = [Lg, D, I, P, ctypes.c_char_p, I]
        L.laghos_host_basis_at.restype = I
        L.laghos_host_basis_at.argtypes = [I, I, D, P, P, P]
        L.laghos_host_locate_initial.restype = I
        L.laghos_host_locate_initial.argtypes = [I, P, P, P, P, P]
        L.laghos_host_write_vti.restype = I
        L.laghos_host_write_vti.argtypes = [ctypes.c_char_p, I, P, P, P, P, Lg, I, D]
        L.laghos_host_history_header.restype = ctypes.c_char_p
        L.laghos_host_history_header.argtypes = []
        L.laghos_host_history_row.restype = I
        L.laghos_host_history_row.argtypes = [Lg, D, D, Lg, Lg, P, D, ctypes.c_char_p, I]
        L.laghos_host_history_write.restype = I
        L.laghos_host_history_write.argtypes = [ctypes.c_char_p, Lg, ctypes.c_char_p, ctypes.POINTER(Lg), ctypes.c_char_p, I]
        L.laghos_host_disc_create.restype = P
        L.laghos_host_disc_create.argtypes = [ctypes.c_char_p, I, I, I, I, D, I, I]
        L.laghos_host_disc_create_renumbered.restype = P
        L.laghos_host_disc_create_renumbered.argtypes = [ctypes.c_char_p, I, I, I, I, D, I, I, ctypes.c_char_p, I]
        L.laghos_host_disc_create_cartesian.restype = P
        L.laghos_host_disc_create_cartesian.argtypes = [I, I, I, I, I, I, I, I, D, I, I, ctypes.c_char_p, I]
        L.laghos_host_disc_destroy.argtypes = [P]
        L.laghos_host_disc_size.restype = Lg
        L.laghos_host_disc_size.argtypes = [P, I]
        L.laghos_host_disc_get.argtypes = [P, I, P]
        _lib = L
    return _lib


def _argv(args):
    arr = (ctypes.c_char_p * len(args))(*[str(a).encode() for a in args])
    return len(args), arr


class Sim:
    """laghos_sim: one simulation on one GPU (one rank)."""

    def __init__(self, args, nranks=1, rank=0, nccl_id=None):
        self.L = load()
        n, arr = _argv(args)
        self.h = self.L.laghos_sim_create(n, arr, nranks, rank, nccl_id)
        if not self.h:
            raise RuntimeError("laghos_sim_create failed (see stderr)")

    def close(self):
        if self.h:
            self.L.laghos_sim_destroy(self.h)
            self.h = None

    def step(self):
        return self.L.laghos_sim_step(self.h)

    def sync(self):
        self.L.laghos_sim_sync(self.h)

    @property
    def t(self):
        return self.L.laghos_sim_time(self.h)

    @property
    def dt(self):
        return self.L.laghos_sim_dt(self.h)

    @property
    def rk_steps(self):
        return self.L.laghos_sim_steps(self.h)

    @property
    def ti(self):
        return self.L.laghos_sim_ti(self.h)

    def e_norm(self):
        return self.L.laghos_sim_enorm(self.h)

    def energy(self):
        return self.L.laghos_sim_energy(self.h)

    def diagnostics(self):
        """The conserved integrals, extremes and bad-point counts of the state as it stands (lgh_diagnostics; what a row of
        the `-hist` file is made of), as a dict by name; every rank calls it."""
        from .context import DIAG_COUNT, diagnostics_dict
        out = np.full(DIAG_COUNT, np.nan)   # (an entry the library did not write would show)
        self.L.laghos_sim_diagnostics(self.h, out.ctypes.data)
        return diagnostics_dict(out)

    def profile(self, axis, nbins, lo, hi, origin=None):
        """The state as it stands binned along x, y, z or the distance r from `origin` (lgh_profile; what a `-prof` file is
        made of): the dict of Context.profile; every rank calls it."""
        from .context import PROFILE_AXES, PROFILE_COLS, PROFILE_MAX_BINS, profile_dict
        o = np.zeros(3)
        if origin is not None:
            g = np.asarray(origin, dtype=np.float64).reshape(-1)[:3]
            o[:g.size] = g
        rows = np.full((max(0, min(int(nbins), PROFILE_MAX_BINS)) + 2, len(PROFILE_COLS)), np.nan)
        n_excl = ctypes.c_long(-1)
        rc = self.L.laghos_sim_profile(self.h, int(PROFILE_AXES.get(axis, axis)), int(nbins), float(lo), float(hi), o.ctypes.data,
                                       rows.ctypes.data, ctypes.byref(n_excl))
        if rc != 0:
            raise RuntimeError(f"laghos_sim_profile: error {rc}: {self.L.laghos_sim_error(self.h).decode()}")
        return profile_dict(rows, n_excl.value, float(lo), float(hi))

    def map(self, cells, lo, hi):
        """The state as it stands binned onto a fixed Cartesian grid of `cells` per axis over the box [lo, hi) (lgh_map; what a
        `-map` file is made of): the dict of Context.map; every rank calls it."""
        from .context import MAP_COLS, map_dict, map_spec
        n, a, b, n_rows = map_spec(cells, lo, hi)
        rows = np.full((n_rows, len(MAP_COLS)), np.nan)
        n_excl = ctypes.c_long(-1)
        na, la, ha = np.asarray(n, dtype=np.int32), np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        rc = self.L.laghos_sim_map(self.h, na.ctypes.data, la.ctypes.data, ha.ctypes.data, rows.ctypes.data, ctypes.byref(n_excl))
        if rc != 0:
            raise RuntimeError(f"laghos_sim_map: error {rc}: {self.L.laghos_sim_error(self.h).decode()}")
        return map_dict(rows, n_excl.value, self.sizes()["dim"], n, a, b)

    def loads(self, planes=()):
        """The pressure loads of the state as it stands on the rows of a `-loads` file (lgh_loads): the boundary of the global
        mesh, its walls, and the planes given as (axis "x" | "y" | "z", K) in their order - the dict of HydroOperator.loads;
        every rank calls it."""
        from .context import LOADS_COLS, loads_dict
        dim = self.sizes()["dim"]
        pl = np.asarray([("xyz".index(a), int(K)) for a, K in planes], dtype=np.int32).reshape(-1, 2)
        names = ["surface"] + [f"{'xyz'[f // 2]}{f % 2}" for f in range(2 * dim)] + [f"plane_{a}{int(K)}" for a, K in planes]
        rows = np.full((len(names), len(LOADS_COLS)), np.nan)
        n_excl = ctypes.c_long(-1)
        rc = self.L.laghos_sim_loads(self.h, len(pl), pl.ctypes.data if len(pl) else None, rows.ctypes.data, ctypes.byref(n_excl))
        if rc != 0:
            raise RuntimeError(f"laghos_sim_loads: error {rc}: {self.L.laghos_sim_error(self.h).decode()}")
        return loads_dict(names, rows, n_excl.value, dim)

    def gauges(self, points):
        """The rows of a `-gauges` file for the state as it stands at gauges given by their positions in the initial mesh (one
        sequence of dim numbers each): (n, 12) by GAUGES_FILE_COLUMNS[3:] - one un-buffered evaluation, as `loads`; every rank calls it."""
        dim = self.sizes()["dim"]
        pts = np.zeros((len(points), 3))
        for g, X in enumerate(points):
            assert len(X) == dim, (X, dim)
            pts[g, :dim] = X
        rows = np.full((len(points), len(GAUGES_FILE_COLUMNS) - 3), np.nan)
        rc = self.L.laghos_sim_gauges(self.h, len(points), pts.ctypes.data, rows.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"laghos_sim_gauges: error {rc}: {self.L.laghos_sim_error(self.h).decode()}")
        return rows

    def derived_fields(self, R):
        """The derived fields of the state as it stands on the lattice of R cells per zone and direction (lgh_sample_derived;
        what `-pv-fields` adds to a dump): a dict detj, div_v, sound_speed (NP), grad_v (dim^2, NP; entry i*dim + j = dv_i/dx_j)
        and, in 2D and 3D, vorticity (NP or (3, NP)), NP = NE (R+1)^dim, zones in the caller's order."""
        sz = self.sizes()
        dim, NP = sz["dim"], sz["NE"] * (R + 1) ** sz["dim"]
        # NaN-filled: an entry the library did not write would show
        out = dict(detj=np.full(NP, np.nan), grad_v=np.full((dim * dim, NP), np.nan), div_v=np.full(NP, np.nan))
        if dim > 1:
            out["vorticity"] = np.full(NP if dim == 2 else (3, NP), np.nan)
        out["sound_speed"] = np.full(NP, np.nan)
        vort = out["vorticity"].ctypes.data if dim > 1 else None
        rc = self.L.laghos_sim_derived_fields(self.h, int(R), out["detj"].ctypes.data, out["grad_v"].ctypes.data, out["div_v"].ctypes.data, vort,
                                              out["sound_speed"].ctypes.data)
        if rc != 0:
            raise RuntimeError(f"laghos_sim_derived_fields: error {rc}: {self.L.laghos_sim_error(self.h).decode()}")
        return out

    def select_faces(self, which):
        """The faces of this rank's zones a dump of the driver holds: which = "surface" (`-pv-surface`: the boundary of the global
        mesh) or (axis, K) with axis "x", "y", "z" (`-pv-slice`); (nfaces, 2) ints (zone, local face) in ascending order."""
        kind, axis, K = (0, 0, 0) if which == "surface" else (1, "xyz".index(which[0]), int(which[1]))
        n = self.L.laghos_sim_select_faces(self.h, kind, axis, K, None)
        if n < 0:
            raise RuntimeError(self.L.laghos_sim_error(self.h).decode())
        faces = np.zeros((n, 2), np.int32)
        if n:
            self.L.laghos_sim_select_faces(self.h, kind, axis, K, faces.ctypes.data)
        return faces

    def face_fields(self, R, which):
        """The state as it stands on the face lattices of R cells per direction of a surface or slice dump (lgh_sample_faces; what
        `-pv-surface` / `-pv-slice` write): which as select_faces takes it, or an (nfaces, 2) array of faces.  A dict of numpy
        arrays over NPt = nfaces (R+1)^(dim-1) points: x, v, area_normal (dim, NPt), e, rho, p, detj, div_v, sound_speed (NPt), grad_v
        (dim^2, NPt), vorticity (NPt in 2D, (3, NPt) in 3D), and faces."""
        faces = self.select_faces(which) if (isinstance(which, str) or isinstance(which[0], str)) else \
            np.ascontiguousarray(np.asarray(which, dtype=np.int32).reshape(-1, 2))
        dim = self.sizes()["dim"]
        nf = faces.shape[0]
        NPt = nf * (R + 1) ** (dim - 1)
        nv = 3 if dim == 3 else 1
        blocks = [("x", dim), ("v", dim), ("e", 1), ("rho", 1), ("p", 1), ("detj", 1), ("grad_v", dim * dim), ("div_v", 1), ("vorticity", nv),
                  ("sound_speed", 1), ("area_normal", dim)]
        buf = np.full(sum(c for _, c in blocks) * NPt, np.nan)   # (an entry the library did not write would show)
        if self.L.laghos_sim_face_fields(self.h, int(R), nf, faces.ctypes.data if nf else None, buf.ctypes.data if nf else None) != 0:
            raise RuntimeError(f"laghos_sim_face_fields: {self.L.laghos_sim_error(self.h).decode()}")
        out, pos = {}, 0
        for k, c in blocks:
            a = buf[pos:pos + c * NPt]
            out[k] = a.reshape(c, NPt).copy() if c > 1 else a.copy()
            pos += c * NPt
        out["faces"] = faces
        return out

    CONTOUR_EXTRA = {"div_v": 1, "vorticity": 2, "grad_v": 4, "detj": 8, "sound_speed": 16}   # the driver's -pv-fields bits

    def contour(self, R, field, value=None, fields=None):
        """A contour of the state as it stands, formed on the lattice of R cells per direction as `-pv-iso` / `-pv-plane` form it
        (LagrangianHydroOperator::Contour): `field` = `value` for density, energy, pressure, speed, x, y, z, div_v, detj or
        sound_speed, or field = ("plane", normal, d).  This rank's primitives as a dict: points (dim, nv), cells (nprim, dim), zone,
        v (dim, nv), e, rho, p (nv), the derived arrays named in `fields` (grad_v (dim^2, nv), vorticity (nv) or (3, nv)), and
        n_skipped; nv = dim * nprim, vertex j of primitive q at dim q + j."""
        dim = self.sizes()["dim"]
        coef = None
        if not isinstance(field, str):
            field, normal, value = field
            coef = np.zeros(3)
            coef[:len(normal)] = normal
            if len(normal) != dim:
                raise RuntimeError(f"contour: a plane of a {dim}D mesh has {dim} normal components")
        fields = tuple(fields or ())
        mask = sum(self.CONTOUR_EXTRA[k] for k in fields)
        ns = ctypes.c_long(-1)
        n = self.L.laghos_sim_contour(self.h, int(R), str(field).encode(), coef.ctypes.data if coef is not None else None, float(value), mask,
                                      ctypes.byref(ns))
        if n < 0:
            raise RuntimeError(f"laghos_sim_contour: {self.L.laghos_sim_error(self.h).decode()}")
        nv, nvort = dim * n, 3 if dim == 3 else 1
        blocks = [("points", dim), ("v", dim), ("e", 1), ("rho", 1), ("p", 1), ("detj", 1), ("grad_v", dim * dim), ("div_v", 1), ("vorticity", nvort),
                  ("sound_speed", 1)]
        buf, zone = np.full(sum(c for _, c in blocks) * nv, np.nan), np.zeros(n, np.int32)
        if self.L.laghos_sim_contour_get(self.h, buf.ctypes.data if n else None, zone.ctypes.data if n else None) != 0:
            raise RuntimeError(f"laghos_sim_contour_get: {self.L.laghos_sim_error(self.h).decode()}")
        out, pos = {}, 0
        for k, c in blocks:
            if k in ("points", "v", "e", "rho", "p") or k in fields:
                a = buf[pos:pos + c * nv]
                out[k] = a.reshape(c, nv).copy() if c > 1 else a.copy()
            pos += c * nv
        out.update(cells=np.arange(nv, dtype=np.int64).reshape(n, dim), zone=zone, n_skipped=ns.value)
        return out

    def sedov_error(self):
        """`-err`: L2 error of the density against the exact Sedov solution at t_final."""
        return self.L.laghos_sim_sedov_error(self.h)

    def enable_timers(self, on):
        self.L.laghos_sim_enable_timers(self.h, int(on))

    def reset_timers(self):
        self.L.laghos_sim_reset_timers(self.h)

    def timers(self):
        t = (ctypes.c_double * 4)()
        c = (ctypes.c_long * 3)()
        self.L.laghos_sim_timers(self.h, t, c)
        return dict(cgH1=t[0], cgL2=t[1], force=t[2], qdata=t[3], H1iter=c[0], L2iter=c[1], quad_tstep=c[2])

    def sizes(self):
        s = (ctypes.c_long * 16)()
        self.L.laghos_sim_sizes(self.h, s)
        keys = ["dim", "NE", "global_NE", "N", "H1GTV", "L2GTV", "NQ", "D1D", "Q1D", "L1D"]
        out = dict(zip(keys, list(s)[:10]))
        out["pgrid"] = tuple(s[10:13])      # process grid of laghos::Partition
        out["local_ne"] = tuple(s[13:16])   # zones of this rank per axis
        return out

    def state(self):
        n = self.L.laghos_sim_state_size(self.h)
        out = np.empty(n)
        self.L.laghos_sim_get_state(self.h, out.ctypes.data)
        return out

    @property
    def repeats(self):
        """repeated steps so far"""
        return self.L.laghos_sim_repeats(self.h)

    def checks(self):
        """`-chk`: (cycles compared so far, all of them passed)"""
        c = (ctypes.c_int * 2)()
        self.L.laghos_sim_checks(self.h, c)
        return c[0], bool(c[1])

    def fingerprint(self):
        """The state fingerprint `-fp` prints, as (sum word, xor word): on one rank lgh_vec_fingerprint of S at offset 0,
        on several ranks the rank-ordered combination (every rank calls it)."""
        out = (ctypes.c_ulonglong * 2)()
        if self.L.laghos_sim_fingerprint(self.h, out) != 0:
            raise RuntimeError(self.L.laghos_sim_error(self.h).decode())
        return int(out[0]), int(out[1])

    def checkpoint(self, stem):
        """A checkpoint of the sim as it stands between two steps: the file `stem` (`stem.<rank>` on several ranks, every
        rank calls it), which `-restart stem` reads.  Returns the path of this rank's piece."""
        if self.L.laghos_sim_write_checkpoint(self.h, str(stem).encode()) != 0:
            raise RuntimeError(self.L.laghos_sim_error(self.h).decode())
        return str(stem)

    RECORD_COLS = ("p_max", "t_p_max", "impulse", "p_last", "rho_max", "speed_max", "e_max", "t_arrival")   # lgh_records_update

    def records(self, which):
        """The `-peaks` records as they stand at a point set of the run: which = "volume" (the lattice of `-paraview`), or as
        select_faces takes it ("surface", (axis, K)).  A dict of the seven arrays a dump holds - peak_pressure, peak_pressure_time,
        pressure_impulse, peak_density, peak_speed, peak_energy, arrival_time (-1 where the threshold was not reached, or none was
        given) - over the points of that dump, and "time", the time of the last update."""
        tag = which if isinstance(which, str) else f"slice_{which[0]}{int(which[1])}"
        t = ctypes.c_double(np.nan)
        n = self.L.laghos_sim_records(self.h, tag.encode(), None, ctypes.byref(t))
        if n < 0:
            raise RuntimeError(self.L.laghos_sim_error(self.h).decode())
        buf = np.full((len(self.RECORD_COLS), n), np.nan)   # (an entry the library did not write would show)
        if n:
            self.L.laghos_sim_records(self.h, tag.encode(), buf.ctypes.data, None)
        names = {"p_max": "peak_pressure", "t_p_max": "peak_pressure_time", "impulse": "pressure_impulse", "rho_max": "peak_density",
                 "speed_max": "peak_speed", "e_max": "peak_energy", "t_arrival": "arrival_time"}
        out = {names[c]: buf[k].copy() for k, c in enumerate(self.RECORD_COLS) if c in names}
        out["time"] = t.value
        return out


class RecordsSidecarError(RuntimeError):
    """A records sidecar that was refused: .code is the RecordsSidecarError of records_sidecar.hpp, the text names the file and the check."""

    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def host_write_records_sidecar(path, state_fp, ti, time, R, threshold, sets):
    """records_sidecar.hpp WriteRecordsSidecar through the host probe: state_fp = (word, word), threshold a number or None, sets a
    list of (tag, block) with block a float64 array (8, points)."""
    L = load()
    fp = np.array(state_fp, dtype=np.uint64)
    blocks = [_f64(b).reshape(8, -1) for _, b in sets]
    pts = np.array([b.shape[1] for b in blocks], dtype=np.int64)
    allb = np.concatenate([b.reshape(-1) for b in blocks]) if blocks else np.zeros(0)
    msg = ctypes.create_string_buffer(1024)
    rc = L.laghos_host_write_records_sidecar(str(path).encode(), fp.ctypes.data, int(ti), float(time), int(R), int(threshold is not None),
                                             0.0 if threshold is None else float(threshold), len(sets), " ".join(t for t, _ in sets).encode(), pts.ctypes.data,
                                             allb.ctypes.data if allb.size else None, msg, len(msg))
    if rc != 0:
        raise RecordsSidecarError(rc, msg.value.decode())


def host_read_records_sidecar(path, capacity_words=1 << 22, capacity_sets=64):
    """records_sidecar.hpp ReadRecordsSidecar through the host probe: a dict state_fp, ti, time, R, threshold (None: none) and sets,
    the list of (tag, block (8, points)); RecordsSidecarError when the file is refused."""
    L = load()
    fp, ints, dbls = np.zeros(2, np.uint64), np.zeros(4, np.int64), np.zeros(2, np.float64)
    tags = ctypes.create_string_buffer(64 * capacity_sets)
    pts, blocks = np.zeros(capacity_sets, np.int64), np.full(capacity_words, np.nan)
    msg = ctypes.create_string_buffer(1024)
    rc = L.laghos_host_read_records_sidecar(str(path).encode(), fp.ctypes.data, ints.ctypes.data, dbls.ctypes.data, tags, len(tags), pts.ctypes.data,
                                            capacity_sets, blocks.ctypes.data, capacity_words, msg, len(msg))
    if rc != 0:
        raise RecordsSidecarError(rc, msg.value.decode())
    sets, pos = [], 0
    for k, tag in enumerate(tags.value.decode().split()):
        n = int(pts[k])
        sets.append((tag, blocks[pos:pos + 8 * n].reshape(8, n).copy()))
        pos += 8 * n
    return dict(state_fp=(int(fp[0]), int(fp[1])), ti=int(ints[0]), time=float(dbls[0]), R=int(ints[1]),
                threshold=float(dbls[1]) if ints[2] else None, sets=sets)


def host_match_records_sidecar(path, state_fp, R, threshold, sets):
    """Reads the sidecar and holds it against what a restarting run expects, as the driver does (MatchRecordsSidecar): sets a list
    of (tag, points).  RecordsSidecarError when it is refused."""
    L = load()
    fp = np.array(state_fp, dtype=np.uint64)
    pts = np.array([n for _, n in sets], dtype=np.int64)
    msg = ctypes.create_string_buffer(1024)
    rc = L.laghos_host_match_records_sidecar(str(path).encode(), fp.ctypes.data, int(R), int(threshold is not None), 0.0 if threshold is None else float(threshold),
                                             len(sets), " ".join(t for t, _ in sets).encode(), pts.ctypes.data, msg, len(msg))
    if rc != 0:
        raise RecordsSidecarError(rc, msg.value.decode())


def host_partition(dim, nx, ny, nz, nranks):
    """Process grid laghos::Partition picks for an nx x ny x nz zone grid (None: not evenly divisible)."""
    L = load()
    pg = (ctypes.c_int * 3)()
    if L.laghos_host_partition(dim, nx, ny, nz, nranks, pg) != 0:
        return None
    return tuple(pg)


def host_tables(order_v, order_e):
    L = load()
    D, Ld = order_v + 1, order_e + 1
    Q = (3 * order_v + order_e - 1) // 2 + 1
    qp, qw, gll = np.empty(Q), np.empty(Q), np.empty(D)
    B, G, Bl = np.empty(Q * D), np.empty(Q * D), np.empty(Q * Ld)
    q = L.laghos_host_tables(order_v, order_e, qp.ctypes.data, qw.ctypes.data, gll.ctypes.data,
                             B.ctypes.data, G.ctypes.data, Bl.ctypes.data)
    assert q == Q
    return dict(qpts=qp, qwts=qw, gll=gll, B=B.reshape(D, Q).T, G=G.reshape(D, Q).T, Bl=Bl.reshape(Ld, Q).T)


def host_lattice_tables(order_v, order_e, R):
    """The 1-D bases at the lattice abscissae r/R, r = 0..R, of the visualisation sampling (Context.sample_fields):
    (B_h1_lat (R+1, order_v+1), B_l2_lat (R+1, order_e+1)), indexed [r, d]."""
    L = load()
    R1, D, Ld = R + 1, order_v + 1, order_e + 1
    Bh, Bl = np.empty(R1 * D), np.empty(R1 * Ld)
    if L.laghos_host_lattice_tables(order_v, order_e, R, Bh.ctypes.data, Bl.ctypes.data) != 0:
        raise ValueError(f"host_lattice_tables({order_v}, {order_e}, {R})")
    return Bh.reshape(D, R1).T, Bl.reshape(Ld, R1).T


def host_lattice_grad_table(order_v, R):
    """The derivatives of the 1-D H1 basis at the lattice abscissae r/R (Context.sample_derived): (R+1, order_v+1), indexed [r, d]."""
    R1, D = R + 1, order_v + 1
    G = np.empty(R1 * D)
    if load().laghos_host_lattice_grad_table(order_v, R, G.ctypes.data) != 0:
        raise ValueError(f"host_lattice_grad_table({order_v}, {R})")
    return G.reshape(D, R1).T


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def host_write_vtu(directory, dim, NE, R1, x, v, e, rho, p, cycle, time, rank=0, nranks=1):
    """One `-paraview` piece from sampled host arrays in the layout of lgh_sample_fields (x, v: dim * NE * R1^dim, the others
    NE * R1^dim); returns the path written, <directory>/cycle_<6 digits>[.<rank>].vtu."""
    L = load()
    arrs = [_f64(a) for a in (x, v, e, rho, p)]
    NP = NE * R1 ** dim
    assert [a.size for a in arrs] == [dim * NP, dim * NP, NP, NP, NP]
    if L.laghos_host_write_vtu(str(directory).encode(), dim, NE, R1, *[a.ctypes.data for a in arrs], cycle, time, rank, nranks) != 0:
        raise RuntimeError(f"cannot write a .vtu under {directory}")
    tag = f"cycle_{cycle:06d}" + (f".{rank}" if nranks > 1 else "")
    return os.path.join(str(directory), tag + ".vtu")


def host_write_vti(directory, dim, cells, lo, hi, rows, n_excluded, cycle, time):
    """One `-map` file from the (ncells + 1, 11) rows of lgh_map (Context.map's `rows`) on the grid of `cells` over [lo, hi)
    (map_spec's forms); returns the path written, <directory>/cycle_<6 digits>.vti."""
    from .context import MAP_COLS, map_spec
    L = load()
    n, a, b, n_rows = map_spec(cells, lo, hi)
    rows = _f64(rows)
    assert rows.size == n_rows * len(MAP_COLS) and all(k == 1 for k in n[dim:])
    na, la, ha = np.asarray(n, dtype=np.int32), _f64(a), _f64(b)
    if L.laghos_host_write_vti(str(directory).encode(), dim, na.ctypes.data, la.ctypes.data, ha.ctypes.data, rows.ctypes.data, int(n_excluded),
                               cycle, time) != 0:
        raise RuntimeError(f"cannot write a .vti under {directory}")
    return os.path.join(str(directory), f"cycle_{cycle:06d}.vti")


def _extra_args(extra, NP=None):
    """(n, names, comps, data pointers, the arrays kept alive) of a list of (name, components, array) for the *_fields writers"""
    n = len(extra)
    arrs = [None if a is None else _f64(a).reshape(-1) for _, _, a in extra]
    if NP is not None:
        assert all(a is not None and a.size == NP * int(c) for (_, c, _), a in zip(extra, arrs))
    names = (ctypes.c_char_p * max(n, 1))(*[str(k).encode() for k, _, _ in extra])
    comps = (ctypes.c_int * max(n, 1))(*[int(c) for _, c, _ in extra])
    data = (ctypes.c_void_p * max(n, 1))(*[None if a is None else a.ctypes.data for a in arrs])
    return n, names, comps, data, arrs


def host_write_vtu_fields(directory, dim, NE, R1, x, v, e, rho, p, extra, cycle, time, rank=0, nranks=1):
    """host_write_vtu with further PointData arrays behind the four standing ones: extra = [(name, components, array)], each
    array NE * R1^dim * components doubles, point by point ((NP, components) in numpy's order)."""
    L = load()
    arrs = [_f64(a) for a in (x, v, e, rho, p)]
    NP = NE * R1 ** dim
    assert [a.size for a in arrs] == [dim * NP, dim * NP, NP, NP, NP]
    n, names, comps, data, keep = _extra_args(extra, NP)
    if L.laghos_host_write_vtu_fields(str(directory).encode(), dim, NE, R1, *[a.ctypes.data for a in arrs], n, names, comps, data, cycle, time,
                                      rank, nranks) != 0:
        raise RuntimeError(f"cannot write a .vtu under {directory}")
    tag = f"cycle_{cycle:06d}" + (f".{rank}" if nranks > 1 else "")
    return os.path.join(str(directory), tag + ".vtu")


def host_write_pvtu_fields(directory, cycle, time, nranks, extra):
    """host_write_pvtu whose pieces carry the extra arrays: extra = [(name, components)] (a third entry is ignored)."""
    n, names, comps, _, _ = _extra_args([(e[0], e[1], None) for e in extra])
    if load().laghos_host_write_pvtu_fields(str(directory).encode(), cycle, time, nranks, n, names, comps) != 0:
        raise RuntimeError(f"cannot write a .pvtu under {directory}")
    return os.path.join(str(directory), f"cycle_{cycle:06d}.pvtu")


def host_write_vtu_faces(directory, dim, faces, R1, x, v, e, rho, p, extra, area_normal, cycle, time, rank=0, nranks=1):
    """One `-pv-surface` / `-pv-slice` piece from sampled host arrays in the layout of lgh_sample_faces: faces (nfaces, 2) ints, x, v,
    area_normal dim * NPt, the others NPt = nfaces * R1^(dim-1); extra as host_write_vtu_fields takes it.  No faces: an empty piece.
    Returns the path written."""
    L = load()
    f = np.ascontiguousarray(np.asarray(faces, dtype=np.int32).reshape(-1, 2))
    NPt = f.shape[0] * R1 ** (dim - 1)
    arrs = [_f64(a).reshape(-1) for a in (x, v, e, rho, p, area_normal)]
    assert [a.size for a in arrs] == [dim * NPt, dim * NPt, NPt, NPt, NPt, dim * NPt]
    n, names, comps, data, keep = _extra_args(extra, NPt)
    ptr = lambda a: a.ctypes.data if a.size else None
    if L.laghos_host_write_vtu_faces(str(directory).encode(), dim, f.shape[0], ptr(f), R1, *[ptr(a) for a in arrs[:5]], n, names, comps, data,
                                     ptr(arrs[5]), cycle, time, rank, nranks) != 0:
        raise RuntimeError(f"cannot write a face .vtu under {directory}")
    tag = f"cycle_{cycle:06d}" + (f".{rank}" if nranks > 1 else "")
    return os.path.join(str(directory), tag + ".vtu")


def host_write_pvtu_faces(directory, cycle, time, nranks, extra):
    """The .pvtu of such pieces: extra = [(name, components)] (a third entry is ignored)."""
    n, names, comps, _, _ = _extra_args([(e[0], e[1], None) for e in extra])
    if load().laghos_host_write_pvtu_faces(str(directory).encode(), cycle, time, nranks, n, names, comps) != 0:
        raise RuntimeError(f"cannot write a .pvtu under {directory}")
    return os.path.join(str(directory), f"cycle_{cycle:06d}.pvtu")


def host_write_vtu_contour(directory, dim, zone, x, v, e, rho, p, extra, iso_value, cycle, time, rank=0, nranks=1):
    """One `-pv-iso` / `-pv-plane` piece from host arrays in the layout of LagrangianHydroOperator::Contour: zone (nprims) ints, x, v
    dim * nv doubles, the others nv = dim * nprims; extra as host_write_vtu_fields takes it.  No primitives: an empty piece.
    Returns the path written."""
    L = load()
    z = np.ascontiguousarray(np.asarray(zone, dtype=np.int32).reshape(-1))
    nv = z.size * dim
    arrs = [_f64(a).reshape(-1) for a in (x, v, e, rho, p)]
    assert [a.size for a in arrs] == [dim * nv, dim * nv, nv, nv, nv]
    n, names, comps, data, keep = _extra_args(extra, nv)
    ptr = lambda a: a.ctypes.data if a.size else None
    if L.laghos_host_write_vtu_contour(str(directory).encode(), dim, z.size, ptr(z), *[ptr(a) for a in arrs], n, names, comps, data, float(iso_value),
                                       cycle, time, rank, nranks) != 0:
        raise RuntimeError(f"cannot write a contour .vtu under {directory}")
    tag = f"cycle_{cycle:06d}" + (f".{rank}" if nranks > 1 else "")
    return os.path.join(str(directory), tag + ".vtu")


def host_write_pvtu_contour(directory, cycle, time, nranks, extra):
    """The .pvtu of such pieces: extra = [(name, components)] (a third entry is ignored)."""
    n, names, comps, _, _ = _extra_args([(e[0], e[1], None) for e in extra])
    if load().laghos_host_write_pvtu_contour(str(directory).encode(), cycle, time, nranks, n, names, comps) != 0:
        raise RuntimeError(f"cannot write a .pvtu under {directory}")
    return os.path.join(str(directory), f"cycle_{cycle:06d}.pvtu")


def host_write_pvtu(directory, cycle, time, nranks):
    """<directory>/cycle_<6 digits>.pvtu naming the pieces of all ranks; returns its path."""
    if load().laghos_host_write_pvtu(str(directory).encode(), cycle, time, nranks) != 0:
        raise RuntimeError(f"cannot write a .pvtu under {directory}")
    return os.path.join(str(directory), f"cycle_{cycle:06d}.pvtu")


def host_write_pvd(path, rel_dir, times, cycles, nranks=1):
    """The collection `path`: one DataSet per (time, cycle), file = <rel_dir>/cycle_<6 digits>.vtu (.pvtu on several ranks)."""
    t, c = _f64(times), np.ascontiguousarray(cycles, dtype=np.int32)
    assert t.size == c.size
    if load().laghos_host_write_pvd(str(path).encode(), str(rel_dir).encode(), int(t.size), t.ctypes.data, c.ctypes.data, nranks) != 0:
        raise RuntimeError(f"cannot write {path}")


HISTORY_COLUMNS = ("cycle", "t", "dt", "rk_steps", "repeats", "mass", "volume", "ie", "ke", "total", "d_total", "px", "py", "pz", "detj_min",
                   "detj_min_rank", "detj_min_zone", "rho_min", "rho_max", "e_min", "e_max", "p_max", "v_max", "n_inverted", "n_negative_e",
                   "n_nonfinite")


def host_history_header():
    """The first line of a `-hist` file (history.hpp), without its newline."""
    return load().laghos_host_history_header().decode()


def host_history_row(cycle, t, dt, rk_steps, repeats, diag, energy_init):
    """One row of a `-hist` file, with its newline, from the 20 doubles of lgh_diagnostics."""
    d = _f64(diag)
    assert d.size == 20
    buf = ctypes.create_string_buffer(2048)
    n = load().laghos_host_history_row(int(cycle), float(t), float(dt), int(rk_steps), int(repeats), d.ctypes.data, float(energy_init), buf, len(buf))
    if n < 0:
        raise RuntimeError("host_history_row: the row does not fit")
    return buf.value.decode()


def host_history_write(path, rows="", keep_upto=None):
    """The file operations of `-hist` without a GPU: keep_upto None starts `path` anew (header only), an int resumes it as
    `-restart` from that cycle does (later rows and a partial last line dropped; a missing file started anew); the lines of
    `rows` are then appended.  Returns the rows in the file; RuntimeError with the reason when a step fails."""
    n = ctypes.c_long(-1)
    msg = ctypes.create_string_buffer(1024)
    rc = load().laghos_host_history_write(str(path).encode(), -1 if keep_upto is None else int(keep_upto), rows.encode(), ctypes.byref(n), msg, len(msg))
    if rc != 0:
        raise RuntimeError(msg.value.decode())
    return n.value


LOADS_FILE_COLUMNS = ("cycle", "t", "name", "n", "area", "fx", "fy", "fz", "pa", "p_mean", "power", "flux", "xn", "p_min", "p_max")


def host_loads_header():
    """The first line of a `-loads` file (loads_output.hpp), without its newline."""
    return load().laghos_host_loads_header().decode()


def host_loads_text(cycle, t, names, rows):
    """The lines of one cycle of a `-loads` file, each with its newline, from the (len(names), 11) rows of lgh_loads."""
    r = _f64(rows)
    assert r.size == 11 * len(names)
    buf = ctypes.create_string_buffer(512 * max(1, len(names)))
    n = load().laghos_host_loads_text(int(cycle), float(t), " ".join(names).encode(), r.ctypes.data, buf, len(buf))
    if n < 0:
        raise RuntimeError("host_loads_text: the lines do not fit")
    return buf.value.decode()


GAUGES_FILE_COLUMNS = ("cycle", "t", "gauge", "x", "y", "z", "vx", "vy", "vz", "rho", "e", "p", "cs", "detj", "div_v")


def host_gauges_header():
    """The first line of a `-gauges` file (gauges_output.hpp), without its newline."""
    return load().laghos_host_gauges_header().decode()


def host_gauges_text(cycle, t, rows):
    """The lines of one sample of a `-gauges` file, each with its newline, from the (n, 12) rows of lgh_gauges_drain."""
    r = _f64(rows).reshape(-1, 12)
    buf = ctypes.create_string_buffer(512 * max(1, len(r)))
    n = load().laghos_host_gauges_text(int(cycle), float(t), len(r), r.ctypes.data, buf, len(buf))
    if n < 0:
        raise RuntimeError("host_gauges_text: the lines do not fit")
    return buf.value.decode()


def host_basis_at(order_v, order_e, xi):
    """(Bh, Gh, Bl): the 1-D H1 basis, its derivative and the L2 basis at the abscissa xi (fem.hpp BasisAt; the tables of a gauge)."""
    Bh, Gh, Bl = np.empty(order_v + 1), np.empty(order_v + 1), np.empty(order_e + 1)
    if load().laghos_host_basis_at(int(order_v), int(order_e), float(xi), Bh.ctypes.data, Gh.ctypes.data, Bl.ctypes.data) != 0:
        raise ValueError(f"host_basis_at({order_v}, {order_e}, {xi})")
    return Bh, Gh, Bl


def host_gauge_tables(order_v, order_e, xi):
    """The tables Context.gauges_create takes for gauges at the reference coordinates xi (n, dim): Bh, Gh (n, dim, D1D), Bl (n, dim, L1D)."""
    xi = np.asarray(xi, dtype=np.float64)
    n, dim = xi.shape
    Bh, Gh, Bl = np.empty((n, dim, order_v + 1)), np.empty((n, dim, order_v + 1)), np.empty((n, dim, order_e + 1))
    for g in range(n):
        for a in range(dim):
            Bh[g, a], Gh[g, a], Bl[g, a] = host_basis_at(order_v, order_e, xi[g, a])
    return Bh, Gh, Bl


def host_locate_initial(breaks, X):
    """fem.hpp LocateInitial: where the point X lies in the tensor grid with the break points `breaks` (one array per axis) -
    (zone index per axis, xi per axis), or None where the driver refuses the point (outside the mesh, not finite)."""
    dim = len(breaks)
    nbrk = np.array([len(b) for b in breaks], dtype=np.int32)
    brk = np.concatenate([_f64(b) for b in breaks])
    x = _f64(np.asarray(X, dtype=np.float64).reshape(dim))
    ijk, xi = np.zeros(3, dtype=np.int32), np.zeros(3)
    rc = load().laghos_host_locate_initial(dim, nbrk.ctypes.data, brk.ctypes.data, x.ctypes.data, ijk.ctypes.data, xi.ctypes.data)
    return None if rc != 0 else ([int(i) for i in ijk[:dim]], [float(v) for v in xi[:dim]])


def host_loads_write(path, lines="", keep_upto=None):
    """The file operations of `-loads` without a GPU, as host_history_write: start anew or resume as `-restart` from cycle
    keep_upto does, then append `lines` (the lines of a cycle) at once.  Returns lines kept + appends; RuntimeError otherwise."""
    n = ctypes.c_long(-1)
    msg = ctypes.create_string_buffer(1024)
    rc = load().laghos_host_loads_write(str(path).encode(), -1 if keep_upto is None else int(keep_upto), lines.encode(), ctypes.byref(n), msg, len(msg))
    if rc != 0:
        raise RuntimeError(msg.value.decode())
    return n.value


CKPT_INT_KEYS = ("dim", "problem", "order_v", "order_e", "Q1D", "NE", "global_NE", "N", "nranks", "rank", "pgrid0", "pgrid1", "pgrid2",
                 "ode_solver", "cg_max_iter", "ti", "steps", "repeats", "checks", "checks_ok", "header_bytes", "state_words",
                 "paraview_dumps")
CKPT_DBL_KEYS = ("cfl", "cg_tol", "t", "dt", "energy_init")


class CheckpointError(RuntimeError):
    """A checkpoint that was refused: .code is the CheckpointError of checkpoint.hpp, the text names the file and the check."""

    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def fingerprint_host(words, offset=0):
    """lgh_fingerprint_host (exported by the HIP library, needs no GPU): (sum word, xor word) of the 64-bit words of a
    contiguous float64 / int64 / uint64 array, the first at position `offset`."""
    from . import _lib as hip_lib
    a = np.ascontiguousarray(words)
    assert a.dtype.itemsize == 8, a.dtype
    out = (ctypes.c_ulonglong * 2)()
    hip_lib.check(hip_lib.load().lgh_fingerprint_host(ctypes.c_void_p(a.ctypes.data) if a.size else None, int(a.size), int(offset), out))
    return int(out[0]), int(out[1])


def host_write_checkpoint(path, header, S, pv_times=(), pv_cycles=()):
    """checkpoint.hpp WriteCheckpoint through the host probe: header = dict of CKPT_INT_KEYS / CKPT_DBL_KEYS (missing keys 0)
    and "setup_fp" = (word, word); S float64, pv_times float64, pv_cycles int64."""
    L = load()
    ints = np.array([int(header.get(k, 0)) for k in CKPT_INT_KEYS] + [0], dtype=np.int64)
    dbls = np.array([float(header.get(k, 0.0)) for k in CKPT_DBL_KEYS], dtype=np.float64)
    fp = np.array(header.get("setup_fp", (0, 0)), dtype=np.uint64)
    S, t = _f64(S), _f64(pv_times)
    c = np.ascontiguousarray(pv_cycles, dtype=np.int64)
    assert t.size == c.size
    msg = ctypes.create_string_buffer(1024)
    rc = L.laghos_host_write_checkpoint(str(path).encode(), ints.ctypes.data, dbls.ctypes.data, fp.ctypes.data, S.ctypes.data, int(S.size),
                                        t.ctypes.data, c.ctypes.data, int(t.size), msg, len(msg))
    if rc != 0:
        raise CheckpointError(rc, msg.value.decode())


def host_read_checkpoint(path, S, pv_times, pv_cycles):
    """checkpoint.hpp ReadCheckpoint through the host probe, into the caller's arrays (float64, float64, int64; at least as
    large as the file's), which stay untouched when the file is refused (CheckpointError).  Returns the header as a dict."""
    L = load()
    assert S.dtype == np.float64 and pv_times.dtype == np.float64 and pv_cycles.dtype == np.int64
    assert S.flags.c_contiguous and pv_times.flags.c_contiguous and pv_cycles.flags.c_contiguous
    ints, dbls, fps = np.zeros(24, np.int64), np.zeros(5, np.float64), np.zeros(4, np.uint64)
    msg = ctypes.create_string_buffer(1024)
    rc = L.laghos_host_read_checkpoint(str(path).encode(), ints.ctypes.data, dbls.ctypes.data, fps.ctypes.data, S.ctypes.data, int(S.size),
                                       pv_times.ctypes.data, pv_cycles.ctypes.data, int(min(pv_times.size, pv_cycles.size)), msg, len(msg))
    if rc != 0:
        raise CheckpointError(rc, msg.value.decode())
    h = dict(zip(CKPT_INT_KEYS, (int(v) for v in ints)))
    h.update(zip(CKPT_DBL_KEYS, (float(v) for v in dbls)))
    h["setup_fp"], h["state_fp"] = (int(fps[0]), int(fps[1])), (int(fps[2]), int(fps[3]))
    return h


def host_disc(mesh, rs, order_v, order_e, problem, blast_energy=1.0, nranks=1, rank=0, renumber=None, seed=1, zones=None):
    """Arrays of the C++ Discretization for one rank (host only, no GPU); renumber = "mfem" / "random": after
    Discretization::Renumber (`-renumber`), with node_perm / elem_perm in the result.  zones = (nx,), (nx, ny) or
    (nx, ny, nz): a Cartesian grid of that many zones of the unit box (the driver's default mesh) instead of `mesh`."""
    L = load()
    ren = renumber.encode() if renumber else None
    if zones is not None:
        n = list(zones) + [1] * (3 - len(zones))
        h = L.laghos_host_disc_create_cartesian(len(zones), n[0], n[1], n[2], rs, order_v, order_e, problem, blast_energy,
                                                nranks, rank, ren, seed)
    else:
        h = L.laghos_host_disc_create_renumbered(mesh.encode(), rs, order_v, order_e, problem, blast_energy, nranks, rank,
                                                 ren, seed)
    if not h:
        raise RuntimeError("laghos_host_disc_create failed")

    def get(kind, dtype):
        n = L.laghos_host_disc_size(h, kind)
        a = np.empty(max(n, 0), dtype=dtype)
        if n > 0:
            L.laghos_host_disc_get(h, kind, a.ctypes.data)
        return a
    out = dict(h1map=get(0, np.int32), S0=get(1, np.float64), rho0_l2=get(2, np.float64),
               gamma=get(3, np.float64), rho0_q=get(4, np.float64),
               ess=[get(5, np.int32), get(6, np.int32), get(7, np.int32)], owner=get(8, np.float64),
               W=get(9, np.float64), nbr_rank=get(10, np.int32))
    out["nbr_nodes"] = [get(11 + k, np.int32) for k in range(len(out["nbr_rank"]))]
    out["node_perm"], out["elem_perm"] = get(100, np.int32), get(101, np.int32)
    L.laghos_host_disc_destroy(h)
    return out
