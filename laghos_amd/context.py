"""Thin Python handle over the C ABI (include/laghos_hip.h) using torch CUDA
tensors as device memory.  Plumbing only: every method is one C-ABI call.

Used by the GPU parity tests and by bench.py; the product host layer that
mirrors the reference's C++ classes lives in laghos_amd/host/.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import LghConfig, check


def _np_i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _np_f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(t):
    """device pointer of a contiguous float64 CUDA tensor"""
    assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
    return ctypes.c_void_p(t.data_ptr())


def _dbl(a):
    """host pointer of a contiguous float64 numpy array (kept alive by the caller)"""
    assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous
    return a.ctypes.data_as(_lib.c_dbl_p)


def sedov_setup(dim, gamma, rho0, blast_energy, omega=0.0):
    """SedovSol::SedovSol (sedov/sedov_sol.cpp:27-117): the 21-entry parameter block."""
    par = np.zeros(21)
    check(_lib.load().lgh_sedov_setup(int(dim), float(gamma), float(rho0), float(blast_energy), float(omega), _dbl(par)))
    return par


def sedov_shock(par, t):
    """SedovSol::SetTime: (r2, U, rho1, rho2, v2, p2)."""
    out = np.zeros(6)
    check(_lib.load().lgh_sedov_shock(_dbl(par), float(t), _dbl(out)))
    return out


def sedov_eval_point(par, t, r):
    """SedovSol::EvalSol at one radius (host)."""
    rho, v, p = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    check(_lib.load().lgh_sedov_eval_point(_dbl(par), float(t), float(r), ctypes.byref(rho), ctypes.byref(v),
                                           ctypes.byref(p)))
    return rho.value, v.value, p.value


# lgh_diagnostics: slot k of the zone arrays (the first 17) and of the global array (include/laghos_hip.h)
DIAG_NAMES = ("mass", "volume", "ie", "ke", "px", "py", "pz", "detj_min", "rho_min", "rho_max", "e_min", "e_max", "p_max", "v_max",
              "n_inverted", "n_negative_e", "n_nonfinite", "detj_min_zone", "detj_min_rank")
DIAG_ZONE_COUNT, DIAG_COUNT = 17, 20
_DIAG_INTS = ("n_inverted", "n_negative_e", "n_nonfinite", "detj_min_zone", "detj_min_rank")


# lgh_profile: the columns of a row (include/laghos_hip.h) and the axis names of Context.profile
PROFILE_COLS = ("n", "vol", "mass", "ie", "ke", "mom", "pv", "mxi", "rho_min", "rho_max")
PROFILE_MAX_BINS = 4096
PROFILE_AXES = {"x": 0, "y": 1, "z": 2, "r": 3}


def profile_dict(rows, n_excluded, lo, hi):
    """what Context.profile returns, from the (nbins + 2, 10) rows of lgh_profile: the raw rows, the bin edges and the
    derived curves of the inner rows - rho = mass / vol, e = ie / mass, v = mom / mass, p = pv / vol, xi = mxi / mass, NaN
    where the divisor is 0"""
    nbins = rows.shape[0] - 2
    inner = rows[1:-1]
    col = {k: inner[:, i] for i, k in enumerate(PROFILE_COLS)}

    def ratio(a, b):
        out = np.full(nbins, np.nan)
        np.divide(a, b, out=out, where=(b != 0))
        return out
    return dict(rows=rows, n_excluded=int(n_excluded), edges=lo + (hi - lo) * np.arange(nbins + 1) / nbins,
                rho=ratio(col["mass"], col["vol"]), e=ratio(col["ie"], col["mass"]), v=ratio(col["mom"], col["mass"]),
                p=ratio(col["pv"], col["vol"]), xi=ratio(col["mxi"], col["mass"]))


# lgh_map: the columns of a row (include/laghos_hip.h)
MAP_COLS = ("n", "vol", "mass", "ie", "ke", "mom_x", "mom_y", "mom_z", "pv", "rho_min", "rho_max")
MAP_MAX_CELLS = 1 << 20


def map_spec(cells, lo, hi):
    """cells, lo, hi of a map - a number, or one per axis - as three lists of 3 (1 cell over [0, 1] on an axis not given) and
    the number of rows a buffer for the call needs (1 for a grid the library refuses)"""
    n = [int(k) for k in np.atleast_1d(cells)][:3]
    a = [float(x) for x in np.atleast_1d(lo)][:3]
    b = [float(x) for x in np.atleast_1d(hi)][:3]
    n, a, b = n + [1] * (3 - len(n)), a + [0.0] * (3 - len(a)), b + [1.0] * (3 - len(b))
    ncells = 1
    for k in n:
        ncells = ncells * k if 1 <= k and 1 <= ncells * k <= MAP_MAX_CELLS else 0
    return n, a, b, ncells + 1


def map_dict(rows, n_excluded, dim, n, lo, hi):
    """what Context.map returns, from the (ncells + 1, 11) rows of lgh_map: the raw rows, `outside` (row 0), `grid` (the other
    rows as (n2, n1, n0, 11)), the cell edges per used axis and the derived rho = mass / vol, e = ie / mass, v = mom / mass
    ((n2, n1, n0, dim)) and p = pv / vol of the cells, NaN where the divisor is 0"""
    grid = rows[1:].reshape(n[2], n[1], n[0], len(MAP_COLS))
    col = {k: grid[..., i] for i, k in enumerate(MAP_COLS)}

    def ratio(a, b):
        b = b.reshape(b.shape + (1,) * (a.ndim - b.ndim))   # (one divisor for the components of a vector)
        out = np.full(a.shape, np.nan)
        np.divide(a, b, out=out, where=(b != 0))
        return out
    return dict(rows=rows, outside=rows[0], grid=grid, n_excluded=int(n_excluded),
                edges=[lo[c] + (hi[c] - lo[c]) * np.arange(n[c] + 1) / n[c] for c in range(dim)],
                rho=ratio(col["mass"], col["vol"]), e=ratio(col["ie"], col["mass"]), v=ratio(grid[..., 5:5 + dim], col["mass"]),
                p=ratio(col["pv"], col["vol"]))


# lgh_loads: the columns of a row (include/laghos_hip.h)
LOADS_COLS = ("n", "area", "force_x", "force_y", "force_z", "pa", "power", "flux", "xn", "p_min", "p_max")
LOADS_MAX_ROWS = 64


def loads_dict(names, rows, n_excluded, dim):
    """what HydroOperator.loads and Sim.loads return, from the (nrows, 11) rows of lgh_loads: the names of the rows, the raw
    rows, `force` (rows[:, 2:2+dim]) and `p_mean` = pa / area, NaN for an empty row"""
    p_mean = np.full(rows.shape[0], np.nan)
    np.divide(rows[:, 5], rows[:, 1], out=p_mean, where=(rows[:, 0] != 0))
    return dict(names=list(names), rows=rows, n_excluded=int(n_excluded), force=rows[:, 2:2 + dim], p_mean=p_mean)


def diagnostics_dict(out):
    """the 20 doubles of lgh_diagnostics by name"""
    return {k: (int(out[i]) if k in _DIAG_INTS else float(out[i])) for i, k in enumerate(DIAG_NAMES)}


def boundary_faces_host(dim, NE, N, D1D, h1_map):
    """lgh_mesh_boundary_faces_host: the faces (zone, local face 2 axis + side) of a mesh given by its element -> node map whose
    D1D^(dim-1) nodes are the node set of no other zone's face, as (nfaces, 2) ints in ascending order.  Needs no GPU."""
    hm = _np_i32(np.asarray(h1_map).reshape(-1))
    assert hm.size == NE * D1D ** dim
    out = np.empty((2 * dim * NE, 2), np.int32)
    n = ctypes.c_int(-1)
    ip = ctypes.POINTER(ctypes.c_int)
    check(_lib.load().lgh_mesh_boundary_faces_host(dim, NE, N, D1D, hm.ctypes.data_as(ip), out.ctypes.data_as(ip), ctypes.byref(n)))
    return out[:n.value].copy()


class Context:
    """lgh_ctx owner.  Arguments follow struct lgh_config: tables are (Q,D)
    arrays B[q,d]; h1_map is (NE, ND); ess is a list of dim int arrays."""

    def __init__(self, dim, NE, D1D, Q1D, L1D, N, h1_map, B_h1, G_h1, B_l2, weights, gamma, ess,
                 owner=None, use_viscosity=True, use_vorticity=False, cfl=0.5, order_v=None,
                 device=0):
        self.lib = _lib.load()
        self.dim, self.NE, self.D1D, self.Q1D, self.L1D, self.N = dim, NE, D1D, Q1D, L1D, N
        self.ND, self.NQ, self.NL = D1D ** dim, Q1D ** dim, L1D ** dim
        self.H1V, self.L2V = dim * N, NE * self.NL
        self.device = torch.device("cuda", device)
        self._gauge_sets = {}   # handle -> (gauges, capacity) of the sets gauges_create made
        keep = dict(
            h1=_np_i32(np.asarray(h1_map).reshape(-1)),
            B=_np_f64(np.asarray(B_h1).T.reshape(-1)),   # -> [q + Q*d]
            G=_np_f64(np.asarray(G_h1).T.reshape(-1)),
            Bl=_np_f64(np.asarray(B_l2).T.reshape(-1)),
            W=_np_f64(weights), gamma=_np_f64(gamma),
            ess=[_np_i32(e) if len(e) else np.zeros(1, np.int32) for e in ess],
            owner=None if owner is None else _np_f64(owner),
        )
        self._keep = keep
        cfg = LghConfig()
        cfg.dim, cfg.NE, cfg.D1D, cfg.Q1D, cfg.L1D, cfg.N = dim, NE, D1D, Q1D, L1D, N
        ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
        cfg.h1_map = keep["h1"].ctypes.data_as(ip)
        cfg.B_h1 = keep["B"].ctypes.data_as(dp)
        cfg.G_h1 = keep["G"].ctypes.data_as(dp)
        cfg.B_l2 = keep["Bl"].ctypes.data_as(dp)
        cfg.weights = keep["W"].ctypes.data_as(dp)
        cfg.gamma = keep["gamma"].ctypes.data_as(dp)
        for k in range(3):
            cfg.ess_count[k] = len(ess[k]) if k < dim else 0
            cfg.ess[k] = keep["ess"][k].ctypes.data_as(ip) if k < dim else None
        cfg.owner = keep["owner"].ctypes.data_as(dp) if owner is not None else None
        cfg.use_viscosity, cfg.use_vorticity = int(use_viscosity), int(use_vorticity)
        cfg.cfl = cfl
        cfg.order_v = order_v if order_v is not None else D1D - 1
        cfg.device = device
        cfg.stream = None
        h = ctypes.c_void_p()
        check(self.lib.lgh_create(ctypes.byref(cfg), ctypes.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.lgh_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- helpers ----------------------------------------------------------------
    def empty(self, n):
        return torch.empty(int(n), dtype=torch.float64, device=self.device)

    # The library works on its own (non-blocking) HIP stream; torch fills tensors on torch's current
    # stream.  A tensor handed to the library must be complete first, so the helpers that WRITE device
    # memory through torch wait for torch's stream before they return (empty() writes nothing).
    def _torch_done(self):
        torch.cuda.current_stream(self.device).synchronize()

    def zeros(self, n):
        t = torch.zeros(int(n), dtype=torch.float64, device=self.device)
        self._torch_done()
        return t

    def to_dev(self, a):
        t = torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(self.device)
        self._torch_done()
        return t

    def clone(self, t):
        """torch clone of a device tensor, complete before the library may touch it"""
        c = t.clone()
        self._torch_done()
        return c

    def sync(self):
        check(self.lib.lgh_sync(self.h))

    def _view(self, ptr, n):
        """read a ctx-owned device array into a numpy array"""
        out = self.empty(n)
        self.sync()
        check(self.lib.lgh_vec_copy(self.h, _ptr(out), ctypes.c_void_p(ptr), int(n)))
        self.sync()
        return out.cpu().numpy()

    def _write(self, ptr, arr):
        t = self.to_dev(arr)
        torch.cuda.synchronize()
        check(self.lib.lgh_vec_copy(self.h, ctypes.c_void_p(ptr), _ptr(t), t.numel()))
        self.sync()

    @property
    def stressJinvT(self):
        return self._view(self.lib.lgh_qdata_stressJinvT(self.h), self.NE * self.NQ * self.dim ** 2)

    def set_stressJinvT(self, arr):
        self._write(self.lib.lgh_qdata_stressJinvT(self.h), arr)

    @property
    def Jac0inv(self):
        return self._view(self.lib.lgh_qdata_Jac0inv(self.h), self.NE * self.NQ * self.dim ** 2)

    @property
    def rho0DetJ0w(self):
        return self._view(self.lib.lgh_qdata_rho0DetJ0w(self.h), self.NE * self.NQ)

    @property
    def massD(self):
        return self._view(self.lib.lgh_mass_D(self.h), self.NE * self.NQ)

    @massD.setter
    def massD(self, arr):
        """overwrite the mass quadrature data (lgh_mass_D is called again after the write: its contract)"""
        self._write(self.lib.lgh_mass_D(self.h), np.ascontiguousarray(arr, dtype=np.float64))
        self.lib.lgh_mass_D(self.h)

    def write_massD_in_place(self, arr):
        """overwrite the table through the pointer as a caller that kept it would (no second lgh_mass_D call);
        lgh_mass_data_changed() is then the caller's duty"""
        if not hasattr(self, "_massD_ptr"):
            self._massD_ptr = self.lib.lgh_mass_D(self.h)
        self._write(self._massD_ptr, np.ascontiguousarray(arr, dtype=np.float64))

    def mass_data_changed(self):
        check(self.lib.lgh_mass_data_changed(self.h))

    @property
    def mass_diag(self):
        return self._view(self.lib.lgh_mass_diag(self.h), self.N)

    # ---- one method per C-ABI entry ------------------------------------------------
    def set_h0(self, h0):
        check(self.lib.lgh_set_h0(self.h, h0))

    def set_dt_est(self, v):
        check(self.lib.lgh_set_dt_est(self.h, v))

    def get_dt_est(self):
        v = ctypes.c_double()
        check(self.lib.lgh_get_dt_est(self.h, ctypes.byref(v)))
        return v.value

    def setup_rho0detj0(self, x0, rho0_l2, rho0_q):
        vol = ctypes.c_double()
        torch.cuda.synchronize()
        check(self.lib.lgh_setup_rho0detj0(self.h, _ptr(x0), _ptr(rho0_l2), _ptr(rho0_q), ctypes.byref(vol)))
        return vol.value

    def force_mult(self, x_l2, y_h1):
        check(self.lib.lgh_force_mult(self.h, _ptr(x_l2), _ptr(y_h1)))

    def force_mult_transpose(self, v_h1, y_l2):
        check(self.lib.lgh_force_mult_transpose(self.h, _ptr(v_h1), _ptr(y_l2)))

    def mass_set_ess(self, comp):
        check(self.lib.lgh_mass_set_essential_tdofs(self.h, comp))

    def mass_eliminate_rhs(self, b):
        check(self.lib.lgh_mass_eliminate_rhs(self.h, _ptr(b)))

    def mass_mult(self, space, x, y, full=False):
        fn = self.lib.lgh_mass_mult_full if full else self.lib.lgh_mass_mult
        check(fn(self.h, space, _ptr(x), _ptr(y)))

    def cg_solve(self, space, b, x, rel_tol, max_iter):
        it = ctypes.c_int(0)
        check(self.lib.lgh_cg_solve(self.h, space, _ptr(b), _ptr(x), rel_tol, max_iter, ctypes.byref(it)))
        return it.value

    def l2_mass_solve_local(self, b, x):
        """1D: x = Me(z)^-1 b zone by zone (the FA energy solve, lgh_l2_mass_solve_local)."""
        check(self.lib.lgh_l2_mass_solve_local(self.h, _ptr(b), _ptr(x)))

    def qupdate(self, S):
        check(self.lib.lgh_qupdate(self.h, _ptr(S)))

    def qupdate_set_tiny_grad(self, v):
        check(self.lib.lgh_qupdate_set_tiny_grad(self.h, float(v)))

    def qupdate_discard(self):
        """(mode, C_F) of lgh_qupdate_discard: which provably unused work the update skips (bit 0 the dt candidate, bit 1 the
        F.1 rows) and the bound constant of the F.1 rows."""
        m, cf = ctypes.c_int(-1), ctypes.c_double(0.0)
        check(self.lib.lgh_qupdate_discard(self.h, ctypes.byref(m), ctypes.byref(cf)))
        return m.value, cf.value

    def table_symmetry(self):
        """(h1, l2): whether lgh_create found the 1-D tables mirror symmetric (plane-form mass kernels need it)."""
        a, b = ctypes.c_int(-1), ctypes.c_int(-1)
        check(self.lib.lgh_table_symmetry(self.h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def k1_form(self):
        """Form of the lockstep velocity solve's mass-apply kernel: 'column', 'plane', 'slab', 'kron' or None."""
        f = ctypes.c_int(-2)
        check(self.lib.lgh_k1_form(self.h, ctypes.byref(f)))
        return {0: "column", 2: "plane", 4: "slab", 5: "kron"}.get(f.value)

    def mesh_order(self):
        """lgh_mesh_order: dict(structured, identity, components, extent) - the library's own zone order / node numbering."""
        o = (ctypes.c_long * 8)()
        check(self.lib.lgh_mesh_order(self.h, o))
        return dict(structured=bool(o[0]), identity=bool(o[1]), components=int(o[2]), extent=(int(o[3]), int(o[4]), int(o[5])))

    def test_vcg_k1(self, r, d_old, rz, rz_prev, first):
        """One launch of the lockstep solve's K1 (lgh_test_vcg_k1): (E-vector planes [3, NE*ND] tensor, den[3])."""
        y = self.empty(3 * self.NE * self.ND)
        rz, rzp, den = _np_f64(rz), _np_f64(rz_prev), np.zeros(3)
        check(self.lib.lgh_test_vcg_k1(self.h, _ptr(r), _ptr(d_old) if d_old is not None else None, _dbl(rz), _dbl(rzp),
                                       int(bool(first)), _ptr(y), _dbl(den)))
        return y.view(3, -1), den

    def test_vcg_merged_faces(self):
        """uint8 mask [NE*ND] of the E-vector entries K1 has already summed into their left x-neighbour's (slab K1, merged
        layout; all zero otherwise) and their number (lgh_test_vcg_merged_faces)."""
        mask = np.zeros(self.NE * self.ND, dtype=np.uint8)
        n = ctypes.c_long(0)
        check(self.lib.lgh_test_vcg_merged_faces(self.h, mask.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n)))
        return mask, n.value

    def test_vcg_k2(self, it, y_E, r, d, x, den, rz, rz_prev, alpha_prev):
        """One launch of the lockstep solve's K2 (lgh_test_vcg_k2); r, d, x are updated in place.
        Returns ((r, z) of the new residual [3], deferred_x)."""
        den, rz, rzp, al, out = _np_f64(den), _np_f64(rz), _np_f64(rz_prev), _np_f64(alpha_prev), np.zeros(3)
        form = ctypes.c_int(-1)
        check(self.lib.lgh_test_vcg_k2(self.h, int(it), _ptr(y_E), _ptr(r), _ptr(d), _ptr(x), _dbl(den), _dbl(rz), _dbl(rzp),
                                       _dbl(al), _dbl(out), ctypes.byref(form)))
        return out, bool(form.value)

    def _exact_sum(self, mode, n, G=0, E=0, scale=None, v=None, w_in=None, w_out=None, d_out=None, i_out=None):
        llp, sc = ctypes.POINTER(ctypes.c_longlong), None if scale is None else np.array([scale], dtype=np.float64)
        check(self.lib.lgh_test_exact_sum(
            self.h, mode, n, int(G), int(E), None if sc is None else _dbl(sc), None if v is None else _dbl(v),
            None if w_in is None else w_in.ctypes.data_as(llp), None if w_out is None else w_out.ctypes.data_as(llp),
            None if d_out is None else _dbl(d_out), None if i_out is None else i_out.ctypes.data_as(_lib.c_int_p)))

    def test_exact_split(self, v, E=0, scale=None):
        """exact_add of every v[i] into zeroed accumulators (lgh_test_exact_sum, mode 0): (limbs int64 [n, 4], accepted bool [n])."""
        v = _np_f64(v)
        limbs, ok = np.zeros((v.size, 4), dtype=np.int64), np.zeros(v.size, dtype=np.int32)
        self._exact_sum(0, v.size, E=E, scale=scale, v=v, w_out=limbs, i_out=ok)
        return limbs, ok != 0

    def test_exact_value(self, limbs, E):
        """exact_value of every row of limbs [n, 4] under E (mode 1): float64 [n]."""
        limbs = np.ascontiguousarray(limbs, dtype=np.int64).reshape(-1, 4)
        out = np.zeros(limbs.shape[0])
        self._exact_sum(1, limbs.shape[0], E=E, w_in=limbs, d_out=out)
        return out

    def test_exact_grid(self, v, G, E=0, scale=None):
        """v [3, n] over G workgroups into a cleared set, then the three folds (mode 2):
        (the set's raw words int64 [56], folds float64 [3 (exact_den, exact_fold, exact_fold_lanes), 3 components])."""
        v = _np_f64(v)
        assert v.ndim == 2 and v.shape[0] == 3
        words, folds = np.zeros(56, dtype=np.int64), np.zeros(9)
        self._exact_sum(2, v.shape[1], G=G, E=E, scale=scale, v=v, w_out=words, d_out=folds)
        return words, folds.reshape(3, 3)

    def test_wave_sum(self, words):
        """wave_sum_i64 of every 64 words (mode 3): what each of the 64 lanes gets, int64, same shape."""
        words = np.ascontiguousarray(words, dtype=np.int64)
        out = np.zeros_like(words)
        self._exact_sum(3, words.size, w_in=words, w_out=out)
        return out

    def test_exact_scale(self, rz):
        """exact_scale of every rz[i] (mode 4): int32 [n]."""
        rz = _np_f64(rz)
        out = np.zeros(rz.size, dtype=np.int32)
        self._exact_sum(4, rz.size, v=rz, i_out=out)
        return out

    def mass_data_form(self):
        """'rank1' when the mass kernels read D[q, e] = W[q] s_e (one double per element), 'stored' otherwise."""
        f = ctypes.c_int(-1)
        check(self.lib.lgh_mass_data_form(self.h, ctypes.byref(f)))
        return "rank1" if f.value == 1 else "stored"

    def jac0inv_form(self):
        """'compact' when the row-form update reads one Jac0inv per zone (lgh_jac0inv_form), 'stored' otherwise."""
        f = ctypes.c_int(-1)
        check(self.lib.lgh_jac0inv_form(self.h, ctypes.byref(f)))
        return "compact" if f.value == 1 else "stored"

    def qupdate_store_stress(self, on):
        """0: lgh_qupdate keeps the stress in registers (stressJinvT is not written; its readers refuse)."""
        check(self.lib.lgh_qupdate_store_stress(self.h, int(bool(on))))

    def set_fused_forces(self, on):
        check(self.lib.lgh_set_fused_forces(self.h, 1 if on else 0))

    def reset_quadrature_data(self):
        check(self.lib.lgh_reset_quadrature_data(self.h))

    def fused_force_mult(self, y_h1):
        """F.1 formed by the last qupdate, summed to the H1 L-vector; False when it is not on hand"""
        return self.lib.lgh_fused_force_mult(self.h, _ptr(y_h1)) == 0

    def fused_force_e(self, y_e):
        """F.1 formed by the last qupdate as E-vector (dim * NE * ND values); False when it is not on hand"""
        return self.lib.lgh_fused_force_e(self.h, _ptr(y_e)) == 0

    def fused_force_mult_transpose(self, y_l2):
        return self.lib.lgh_fused_force_mult_transpose(self.h, _ptr(y_l2)) == 0

    def quadrature_generation(self):
        """(generation, fused F.1 on hand, fused F^T v on hand)"""
        g, a, b = ctypes.c_ulong(0), ctypes.c_int(-1), ctypes.c_int(-1)
        check(self.lib.lgh_quadrature_generation(self.h, ctypes.byref(g), ctypes.byref(a), ctypes.byref(b)))
        return g.value, a.value, b.value

    def solve_velocity(self, S, dS, one, rhs, work, rel_tol, max_iter):
        """one = None: the operator's own constant-one vector (laghos_solver.cpp:170-171)"""
        it = ctypes.c_int(0)
        check(self.lib.lgh_solve_velocity(self.h, _ptr(S), _ptr(dS), _ptr(one) if one is not None else None, _ptr(rhs), _ptr(work),
                                          rel_tol, max_iter, ctypes.byref(it)))
        return it.value

    def solve_energy(self, S, v, dS, e_rhs, rel_tol, max_iter, e_source=None):
        it = ctypes.c_int(0)
        check(self.lib.lgh_solve_energy(self.h, _ptr(S), _ptr(v), _ptr(dS), _ptr(e_rhs),
                                        _ptr(e_source) if e_source is not None else None,
                                        rel_tol, max_iter, ctypes.byref(it)))
        return it.value

    def set_velocity_source(self, accel):
        check(self.lib.lgh_set_velocity_source(self.h, _ptr(accel) if accel is not None else None))

    def tg_source_2d(self, S, out):
        check(self.lib.lgh_tg_source_2d(self.h, _ptr(S), _ptr(out)))

    # ---- `-err`: density against the exact Sedov solution (include/laghos_hip.h) ----
    def compute_density(self, x, rho_l2):
        """ComputeDensity (laghos_solver.cpp:542-563); x = S (positions first)."""
        check(self.lib.lgh_compute_density(self.h, _ptr(x), _ptr(rho_l2)))

    def sedov_eval(self, par, t, r, rho, v, P):
        """SedovSol::EvalSol for a device array of radii."""
        check(self.lib.lgh_sedov_eval(self.h, _dbl(par), float(t), r.numel(), _ptr(r), _ptr(rho), _ptr(v), _ptr(P)))

    def sedov_density_error(self, x, rho_l2, par, t, origin, weights, B_h1, G_h1, B_l2):
        """Integral of (rho_exact - rho_h)^2 over the current mesh (laghos.cpp:1027-1080);
        the tables are host arrays of the error rule: weights[n], B/G [p + n*d], B_l2 [p + n*l]."""
        import numpy as np
        w = np.ascontiguousarray(weights, dtype=np.float64)
        tabs = [np.ascontiguousarray(a, dtype=np.float64).ravel() for a in (B_h1, G_h1, B_l2)]
        org = np.zeros(3)
        org[:len(origin)] = origin
        out = ctypes.c_double()
        check(self.lib.lgh_sedov_density_error(self.h, _ptr(x), _ptr(rho_l2), _dbl(par), float(t), _dbl(org),
                                               int(w.size), _dbl(w), _dbl(tabs[0]), _dbl(tabs[1]), _dbl(tabs[2]),
                                               ctypes.byref(out)))
        return out.value

    def sample_fields(self, S, rho_l2, B_h1_lat, B_l2_lat, x=None, v=None, e=None, rho=None, p=None):
        """lgh_sample_fields: the fields of S (and the density dofs rho_l2, or None) on the lattice whose host tables are
        B_h1_lat (R1, D1D) and B_l2_lat (R1, L1D), indexed [r, d]; x, v: device tensors of dim * NE * R1^dim, e, rho, p:
        NE * R1^dim, each may be None (skipped).  Asynchronous."""
        Bh = _np_f64(np.asarray(B_h1_lat).T.reshape(-1))   # -> [r + R1*d]
        Bl = _np_f64(np.asarray(B_l2_lat).T.reshape(-1))
        R1 = int(np.asarray(B_h1_lat).shape[0])
        opt = lambda t: _ptr(t) if t is not None else None
        check(self.lib.lgh_sample_fields(self.h, _ptr(S), opt(rho_l2), R1, _dbl(Bh), _dbl(Bl), opt(x), opt(v), opt(e), opt(rho),
                                         opt(p)))

    def sample_derived(self, S, B_h1_lat, G_h1_lat, B_l2_lat, detj=None, grad_v=None, div_v=None, vorticity=None, sound_speed=None):
        """lgh_sample_derived: the derived fields of S on the lattice whose host tables are B_h1_lat, G_h1_lat (R1, D1D; values and
        derivatives of the H1 basis) and B_l2_lat (R1, L1D), indexed [r, d]; device tensors of NP = NE * R1^dim (detj, div_v,
        sound_speed), dim^2 * NP (grad_v, entry i*dim + j = dv_i/dx_j) and NP in 2D / 3 * NP in 3D (vorticity), each may be None
        (skipped).  Asynchronous."""
        Bh = _np_f64(np.asarray(B_h1_lat).T.reshape(-1))   # -> [r + R1*d]
        Gh = _np_f64(np.asarray(G_h1_lat).T.reshape(-1))
        Bl = _np_f64(np.asarray(B_l2_lat).T.reshape(-1))
        R1 = int(np.asarray(B_h1_lat).shape[0])
        opt = lambda t: _ptr(t) if t is not None else None
        check(self.lib.lgh_sample_derived(self.h, _ptr(S), R1, _dbl(Bh), _dbl(Gh), _dbl(Bl), opt(detj), opt(grad_v), opt(div_v), opt(vorticity),
                                          opt(sound_speed)))

    def sample_faces(self, S, rho_l2, B_h1_lat, G_h1_lat, B_l2_lat, faces, x=None, v=None, e=None, rho=None, p=None, detj=None, grad_v=None,
                     div_v=None, vorticity=None, sound_speed=None, area_normal=None):
        """lgh_sample_faces: the outputs of sample_fields and sample_derived on the lattices of the zone faces `faces` - (nfaces, 2)
        ints (zone, local face 2 axis + side), a host array - and the outward area vectors; tables as there ([r, d]; None where no
        output needs one); device tensors over NPt = nfaces * R1^(dim-1) points in the layouts of the two volume calls, area_normal
        dim * NPt; each may be None (skipped).  Asynchronous."""
        tab = lambda T: None if T is None else _np_f64(np.asarray(T).T.reshape(-1))   # -> [r + R1*d]
        Bh, Gh, Bl = tab(B_h1_lat), tab(G_h1_lat), tab(B_l2_lat)
        R1 = int(np.asarray(next(T for T in (B_h1_lat, G_h1_lat, B_l2_lat) if T is not None)).shape[0])
        f = np.ascontiguousarray(np.asarray(faces, dtype=np.int32).reshape(-1))
        assert f.size % 2 == 0
        opt = lambda t: _ptr(t) if t is not None else None
        dbl = lambda a: _dbl(a) if a is not None else None
        fp = f.ctypes.data_as(ctypes.POINTER(ctypes.c_int)) if f.size else None
        check(self.lib.lgh_sample_faces(self.h, _ptr(S), opt(rho_l2), R1, dbl(Bh), dbl(Gh), dbl(Bl), f.size // 2, fp, opt(x), opt(v), opt(e),
                                        opt(rho), opt(p), opt(detj), opt(grad_v), opt(div_v), opt(vorticity), opt(sound_speed), opt(area_normal)))

    def faces_per_block(self, R1):
        """lgh_sample_faces_fpb: faces per workgroup of sample_faces on R1 lattice points per direction, for lists long enough."""
        n = ctypes.c_int(-1)
        check(self.lib.lgh_sample_faces_fpb(self.h, int(R1), ctypes.byref(n)))
        return n.value

    def boundary_faces(self):
        """The boundary faces of this context's mesh, (nfaces, 2) ints (zone, local face) in ascending order, found from the
        element -> node map alone (lgh_mesh_boundary_faces_host; no GPU work)."""
        return boundary_faces_host(self.dim, self.NE, self.N, self.D1D, self._keep["h1"])

    def diagnostics_zones(self, S, out):
        """lgh_diagnostics_zones: the 17 zone diagnostics of S into the device tensor out (17 * NE), out[k * NE + z] with z
        the caller's zone id and k the position in DIAG_NAMES.  Asynchronous."""
        assert out.numel() == DIAG_ZONE_COUNT * self.NE
        check(self.lib.lgh_diagnostics_zones(self.h, _ptr(S), _ptr(out)))

    def diagnostics(self, S, raw=False):
        """lgh_diagnostics: the diagnostics of S folded over zones and ranks, as a dict by DIAG_NAMES (counts, the zone and
        its rank as ints), or the 20 doubles themselves (raw=True).  Synchronous."""
        out = np.full(DIAG_COUNT, np.nan)   # (an entry the library did not write would show)
        check(self.lib.lgh_diagnostics(self.h, _ptr(S), _dbl(out)))
        return out if raw else diagnostics_dict(out)

    def profile(self, S, axis, nbins, lo, hi, origin=None):
        """lgh_profile: the flow binned along a coordinate - axis 0, 1, 2 (or "x", "y", "z") or 3 ("r", the distance from
        `origin`) - into nbins uniform bins of [lo, hi): a dict with `rows` ((nbins + 2, 10), PROFILE_COLS; row 0 below lo,
        the last row at or above hi), `n_excluded`, `edges` and the derived rho, e, v, p, xi of the inner rows
        (profile_dict).  Exact, order-free sums: the same bits for every numbering, grid and rank count.  Synchronous."""
        from ._lib import LghProfileSpec
        spec = LghProfileSpec()
        spec.axis, spec.nbins, spec.lo, spec.hi = int(PROFILE_AXES.get(axis, axis)), int(nbins), float(lo), float(hi)
        o = np.zeros(3) if origin is None else np.asarray(origin, dtype=np.float64).reshape(-1)
        for k in range(min(3, o.size)):
            spec.origin[k] = float(o[k])
        n_rows = max(0, min(int(nbins), PROFILE_MAX_BINS)) + 2
        rows = np.full((n_rows, len(PROFILE_COLS)), np.nan)   # (an entry the library did not write would show)
        n_excl = ctypes.c_long(-1)
        check(self.lib.lgh_profile(self.h, _ptr(S), ctypes.byref(spec), _dbl(rows), ctypes.byref(n_excl)))
        return profile_dict(rows, n_excl.value, spec.lo, spec.hi)

    def map(self, S, cells, lo, hi):
        """lgh_map: the flow binned onto a fixed Cartesian grid - `cells` per axis over the box [lo, hi) (a number or one per
        axis of the dimension): a dict with `rows` ((ncells + 1, 11), MAP_COLS), `outside` (row 0: the points beside the box),
        `grid` (the cells as (n2, n1, n0, 11)), `edges`, `n_excluded` and the derived rho, e, v, p of the cells (map_dict).
        Exact, order-free sums: the same bits for every numbering, launch grid and rank count.  Synchronous."""
        from ._lib import LghMapSpec
        n, a, b, n_rows = map_spec(cells, lo, hi)
        spec = LghMapSpec()
        for k in range(3):
            spec.n[k], spec.lo[k], spec.hi[k] = n[k], a[k], b[k]
        rows = np.full((n_rows, len(MAP_COLS)), np.nan)   # (an entry the library did not write would show)
        n_excl = ctypes.c_long(-1)
        check(self.lib.lgh_map(self.h, _ptr(S), ctypes.byref(spec), _dbl(rows), ctypes.byref(n_excl)))
        return map_dict(rows, n_excl.value, self.dim, n, a, b)

    def loads(self, S, rho_l2, faces, nrows):
        """lgh_loads: pressure loads on zone faces - `faces` (nfaces, 3) ints (zone, local face 2 axis + side, row), a host array;
        S and the density dofs rho_l2 device tensors: (rows, n_excluded), rows (nrows, 11) by LOADS_COLS.  Exact, order-free sums:
        the same bits for every face order, numbering, launch grid and rank count.  Synchronous; 2D and 3D."""
        f = np.ascontiguousarray(np.asarray(faces, dtype=np.int32).reshape(-1))
        assert f.size % 3 == 0
        fp = f.ctypes.data_as(ctypes.POINTER(ctypes.c_int)) if f.size else None
        n_rows = max(1, min(int(nrows), LOADS_MAX_ROWS))   # (a buffer also for a count the library refuses)
        rows = np.full((n_rows, len(LOADS_COLS)), np.nan)   # (an entry the library did not write would show)
        n_excl = ctypes.c_long(-1)
        check(self.lib.lgh_loads(self.h, _ptr(S), _ptr(rho_l2) if rho_l2 is not None else None, int(nrows), f.size // 3, fp, _dbl(rows),
                                 ctypes.byref(n_excl)))
        return rows, n_excl.value

    def loads_faces_per_block(self):
        """lgh_loads_fpb: faces per workgroup of `loads`, for lists long enough."""
        n = ctypes.c_int(-1)
        check(self.lib.lgh_loads_fpb(self.h, ctypes.byref(n)))
        return n.value

    # ---- contours of a lattice scalar (include/laghos_hip.h: lgh_contour) ----
    def contour_into(self, scalar, iso, R1, capacity, edges=None, t=None, zone=None):
        """lgh_contour as it is: `scalar` a device tensor on the lattice of sample_fields (NE * R1^dim), room for `capacity`
        primitives in the device tensors edges (int32, 2 dim per primitive), t (float64, dim per primitive) and zone (int32, or
        None); (n_prims, n_skipped).  Nothing is written when n_prims > capacity; capacity 0 without outputs counts."""
        opt = lambda x, ptr: ptr(x) if x is not None else None
        n, ns = ctypes.c_long(-1), ctypes.c_long(-1)
        check(self.lib.lgh_contour(self.h, int(R1), opt(scalar, _ptr), float(iso), int(capacity), opt(edges, self._int_ptr), opt(t, _ptr),
                                   opt(zone, self._int_ptr), ctypes.byref(n), ctypes.byref(ns)))
        return n.value, ns.value

    @staticmethod
    def _int_ptr(x):
        assert x.is_cuda and x.dtype == torch.int32 and x.is_contiguous()
        return ctypes.c_void_p(x.data_ptr())

    def contour(self, scalar, iso, R1):
        """The contour of the lattice scalar at `iso` (marching tetrahedra in 3D, triangles in 2D): the counting call, buffers of
        the size it names, the emitting call.  (edges, t, zone, n_skipped): device tensors edges (n, dim, 2) int32 - the lattice
        edge (p0 < p1) of every vertex -, t (n, dim) float64 - its weight on that edge -, zone (n,) int32, in the fixed order of
        the definition; n_skipped the simplices left out for a value that is not finite.  Synchronous."""
        dim = self.dim
        n, ns = self.contour_into(scalar, iso, R1, 0)
        edges = torch.zeros((n, dim, 2), dtype=torch.int32, device=self.device)
        t = torch.zeros((n, dim), dtype=torch.float64, device=self.device)
        zone = torch.zeros(n, dtype=torch.int32, device=self.device)
        self._torch_done()
        if n:
            assert self.contour_into(scalar, iso, R1, n, edges, t, zone) == (n, ns)
            self.sync()
        return edges, t, zone, ns

    def contour_gather(self, edges, t, field, ncomp=1):
        """lgh_contour_gather: the lattice array `field` (device, ncomp * NP, component-major) at the vertices of a contour,
        a + t (b - a) along each vertex's lattice edge: a device tensor (ncomp, n_verts), vertices in the order of t.reshape(-1).
        Asynchronous."""
        nv = int(t.numel())
        assert edges.numel() == 2 * nv and field.numel() % ncomp == 0
        out = self.empty(ncomp * nv)
        check(self.lib.lgh_contour_gather(self.h, nv, self._int_ptr(edges) if nv else None, _ptr(t) if nv else None, int(ncomp),
                                          field.numel() // ncomp, _ptr(field), _ptr(out) if nv else None))
        return out.reshape(ncomp, nv)

    def contour_scalar(self, mode, block, coef=None, out=None):
        """lgh_contour_scalar: from the lattice block `block` (device, dim * NP: x or v of sample_fields) the scalar
        coef[0] x + coef[1] y (+ coef[2] z) (mode 0 or "plane") or |block| (mode 1 or "norm"), NP values.  Asynchronous."""
        mode = {"plane": 0, "norm": 1}.get(mode, mode)
        NP = block.numel() // self.dim
        c = np.zeros(4)
        if coef is not None:
            c[:len(coef)] = coef
        out = self.empty(NP) if out is None else out
        check(self.lib.lgh_contour_scalar(self.h, int(mode), NP, self.dim, _ptr(block), _dbl(c), _ptr(out)))
        return out

    def contour_zpb(self, R1):
        """lgh_contour_zpb: zones per workgroup of the count and emit kernels of `contour` on R1 lattice points per direction."""
        n = ctypes.c_int(-1)
        check(self.lib.lgh_contour_zpb(self.h, int(R1), ctypes.byref(n)))
        return n.value

    def solve_energy_begin(self, S, v, dS, e_rhs, rel_tol, max_iter, e_source=None):
        check(self.lib.lgh_solve_energy_begin(self.h, _ptr(S), _ptr(v), _ptr(dS), _ptr(e_rhs),
                                              _ptr(e_source) if e_source is not None else None,
                                              rel_tol, max_iter))

    def solve_energy_end(self):
        it = ctypes.c_int(0)
        check(self.lib.lgh_solve_energy_end(self.h, ctypes.byref(it)))
        return it.value

    def vec_axpby(self, z, a, x, b, y):
        check(self.lib.lgh_vec_axpby(self.h, _ptr(z), a, _ptr(x), b, _ptr(y), z.numel()))

    def vec_axpby_pair(self, z1, a1, x1, b1, z2, a2, x2, b2, y):
        check(self.lib.lgh_vec_axpby_pair(self.h, _ptr(z1), a1, _ptr(x1), b1, _ptr(z2), a2, _ptr(x2), b2, _ptr(y), z1.numel()))

    def vec_copy(self, y, x):
        check(self.lib.lgh_vec_copy(self.h, _ptr(y), _ptr(x), y.numel()))

    def vec_dot(self, x, y):
        v = ctypes.c_double()
        check(self.lib.lgh_vec_dot(self.h, _ptr(x), _ptr(y), x.numel(), ctypes.byref(v)))
        return v.value

    def fingerprint(self, t, offset=0):
        """lgh_vec_fingerprint: the two 64-bit words (sum, xor) of the state fingerprint (include/lgh_fingerprint.h) of the
        device tensor t, its first element at position `offset`.  Synchronous; reads t only."""
        out = (ctypes.c_ulonglong * 2)()
        check(self.lib.lgh_vec_fingerprint(self.h, _ptr(t), t.numel(), int(offset), out))
        return int(out[0]), int(out[1])

    def fingerprint_shape(self, t):
        """(workgroups, threads, scalar head, words per pass of the largest grid) of the launch fingerprint(t) makes"""
        out = (ctypes.c_long * 4)()
        check(self.lib.lgh_vec_fingerprint_shape(self.h, _ptr(t), t.numel(), out))
        return tuple(out)

    RECORD_COLS = ("p_max", "t_p_max", "impulse", "p_last", "rho_max", "speed_max", "e_max", "t_arrival")   # LGH_RECORDS_COLS = 8

    def records_update(self, dim, p, rho, e, v, t, dtr, rec, threshold=None, first=False):
        """lgh_records_update: folds the sample p, rho, e (n each) and v (dim * n, component-major) taken at time t, dtr after the
        last update, into the record block rec (8 * n, column-major, RECORD_COLS); threshold None: none; first: start the records
        (dtr must be 0).  All device tensors, each may start at any 8-byte aligned address.  Asynchronous."""
        n = p.numel()
        assert rho.numel() == n and e.numel() == n and v.numel() == dim * n and rec.numel() == len(self.RECORD_COLS) * n
        check(self.lib.lgh_records_update(self.h, n, int(dim), _ptr(p), _ptr(rho), _ptr(e), _ptr(v), float(t), float(dtr),
                                          float("nan") if threshold is None else float(threshold), int(bool(first)), _ptr(rec)))

    def records_shape(self, n):
        """(workgroups, threads, points per lane per trip, trips) of the launch records_update makes for n points"""
        out = (ctypes.c_long * 4)()
        check(self.lib.lgh_records_shape(self.h, int(n), out))
        return tuple(out)

    GAUGE_COLS = ("x", "y", "z", "vx", "vy", "vz", "rho", "e", "p", "cs", "detj", "div_v")   # LGH_GAUGE_COLS = 12

    def gauges_create(self, zone, Bh, Gh, Bl, x0, rho0_l2, capacity=256):
        """lgh_gauges_create: a set of n gauges - material points (zone, xi) - as a handle.  zone: n ints, the caller's zone id on
        this rank or -1; Bh, Gh (n, dim, D1D) and Bl (n, dim, L1D): host arrays of the 1-D H1 values, H1 derivatives and L2
        values at xi per gauge and axis; x0, rho0_l2: device tensors of the initial positions and density dofs (m_g = rho0 detJ0
        is formed from them); capacity: samples the device buffer holds.  Collective on several ranks."""
        z = _np_i32(np.asarray(zone).reshape(-1))
        n = int(z.size)
        tabs = [_np_f64(np.asarray(T, dtype=np.float64).reshape(-1)) for T in (Bh, Gh, Bl)]
        assert tabs[0].size == n * self.dim * self.D1D and tabs[1].size == tabs[0].size and tabs[2].size == n * self.dim * self.L1D
        h = ctypes.c_int(-1)
        check(self.lib.lgh_gauges_create(self.h, n, z.ctypes.data_as(_lib.c_int_p) if n else None, _dbl(tabs[0]), _dbl(tabs[1]), _dbl(tabs[2]),
                                         _ptr(x0), _ptr(rho0_l2), int(capacity), ctypes.byref(h)))
        self._gauge_sets[h.value] = (n, int(capacity))
        return h.value

    def gauges_sample(self, handle, S):
        """lgh_gauges_sample: appends one sample of the state S to the set's buffer.  Asynchronous; refused on a full buffer."""
        check(self.lib.lgh_gauges_sample(self.h, int(handle), _ptr(S)))

    def gauges_pending(self, handle):
        n = ctypes.c_int(-1)
        check(self.lib.lgh_gauges_pending(self.h, int(handle), ctypes.byref(n)))
        return n.value

    def gauges_drain(self, handle):
        """lgh_gauges_drain: the pending samples, oldest first, as (samples, n, 12) by GAUGE_COLS; empties the buffer.
        Synchronous; collective on several ranks (every rank gets every row)."""
        n, cap = self._gauge_sets.get(int(handle), (1, 1))
        out = np.full((cap, n, len(self.GAUGE_COLS)), np.nan)   # (an entry the library did not write would show)
        k = ctypes.c_int(-1)
        check(self.lib.lgh_gauges_drain(self.h, int(handle), _dbl(out), cap, ctypes.byref(k)))
        return out[:k.value].copy()

    def gauges_mass(self, handle):
        """lgh_gauges_mass: m_g = rho0(xi_g) detJ0(xi_g) of this rank's gauges (-0.0 where another rank owns one)"""
        n, _ = self._gauge_sets.get(int(handle), (1, 1))
        out = np.full(n, np.nan)
        check(self.lib.lgh_gauges_mass(self.h, int(handle), _dbl(out)))
        return out

    def gauges_shape(self, handle):
        """(gauges per workgroup, workgroups, LDS bytes of a workgroup, threads) of the launch gauges_sample makes"""
        out = (ctypes.c_long * 4)()
        check(self.lib.lgh_gauges_shape(self.h, int(handle), out))
        return tuple(out)

    def gauges_destroy(self, handle):
        check(self.lib.lgh_gauges_destroy(self.h, int(handle)))
        self._gauge_sets.pop(int(handle), None)

    def internal_energy(self, e):
        v = ctypes.c_double()
        check(self.lib.lgh_internal_energy(self.h, _ptr(e), ctypes.byref(v)))
        return v.value

    def kinetic_energy(self, vel):
        v = ctypes.c_double()
        check(self.lib.lgh_kinetic_energy(self.h, _ptr(vel), ctypes.byref(v)))
        return v.value

    def timers(self):
        t = (ctypes.c_double * 4)()
        c = (ctypes.c_long * 3)()
        check(self.lib.lgh_get_timers(self.h, t, c))
        return dict(cgH1=t[0], cgL2=t[1], force=t[2], qdata=t[3], H1iter=c[0], L2iter=c[1],
                    quad_tstep=c[2])

    def reset_timers(self):
        check(self.lib.lgh_reset_timers(self.h))

    def enable_timers(self, on):
        check(self.lib.lgh_enable_timers(self.h, int(on)))

    # E-level (tests)
    def force_mult_E(self, sJit, xE, yE):
        check(self.lib.lgh_force_mult_E(self.h, _ptr(sJit), _ptr(xE), _ptr(yE)))

    def force_mult_transpose_E(self, sJit, vE, yE):
        check(self.lib.lgh_force_mult_transpose_E(self.h, _ptr(sJit), _ptr(vE), _ptr(yE)))

    def mass_apply_E(self, space, xE, yE):
        check(self.lib.lgh_mass_apply_E(self.h, space, _ptr(xE), _ptr(yE)))

    def test_eig(self, dim, A, lam, vec):
        check(self.lib.lgh_test_eig(self.h, dim, lam.numel(), _ptr(A), _ptr(lam), _ptr(vec)))

    def test_singular(self, dim, A, sv):
        check(self.lib.lgh_test_singular(self.h, dim, sv.numel(), _ptr(A), _ptr(sv)))

    def test_sqrt(self, x, y):
        check(self.lib.lgh_test_sqrt(self.h, y.numel(), _ptr(x), _ptr(y)))

    # multi-GPU
    def comm_init(self, nranks, rank, unique_id):
        check(self.lib.lgh_comm_init(self.h, nranks, rank, unique_id))

    def comm_set_neighbors(self, nbr_rank, nbr_nodes):
        n = len(nbr_rank)
        ranks = _np_i32(nbr_rank) if n else np.zeros(1, np.int32)
        counts = _np_i32([len(x) for x in nbr_nodes]) if n else np.zeros(1, np.int32)
        lists = [_np_i32(x) for x in nbr_nodes]
        ip = ctypes.POINTER(ctypes.c_int)
        arr = (ip * max(n, 1))(*[l.ctypes.data_as(ip) for l in lists])
        check(self.lib.lgh_comm_set_neighbors(self.h, n, ranks.ctypes.data_as(ip), counts.ctypes.data_as(ip), arr))

    def test_word_peers(self, nwords):
        cap = ctypes.c_long(-1)
        check(self.lib.lgh_test_word_peers(self.h, nwords, ctypes.byref(cap)))
        return cap.value

    def test_set_rank(self, nranks, rank):
        check(self.lib.lgh_test_set_rank(self.h, nranks, rank))

    def test_halo_pack(self, v, ncomp, out):
        check(self.lib.lgh_test_halo_pack(self.h, _ptr(v), ncomp, _ptr(out)))

    def test_halo_combine(self, inp, v, ncomp):
        check(self.lib.lgh_test_halo_combine(self.h, _ptr(inp), _ptr(v), ncomp))

    def halo_sum(self, v, ncomp):
        check(self.lib.lgh_halo_sum(self.h, _ptr(v), ncomp))

    def allreduce(self, value, op=0):
        v = ctypes.c_double(value)
        check(self.lib.lgh_allreduce(self.h, ctypes.byref(v), op))
        return v.value


def unique_id():
    buf = ctypes.create_string_buffer(128)
    check(_lib.load().lgh_comm_unique_id(buf))
    return buf.raw
